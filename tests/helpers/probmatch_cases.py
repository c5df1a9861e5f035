"""A CPU model of the bucket mapping, the per-workgroup bucket table and the work split of
pysteps_amd/csrc/probmatch.hip, and named inputs that reach each of its kernel paths at the smallest size.

The model restates, in the kernels' operation order:
  bin_of / bin_i      bucket of a wet value in the target's 2^20 and the initial array's 2^21 buckets, the clamp to
                      the last bucket and the scale of pm_prepare (0 when max - min is not positive)
  hash_home / table   the open-addressing table of pm_hist_target / pm_scatter_target: kHashSlots slots, kProbes
                      linear probes from a multiplicative hash, "no room" for a bucket that finds them taken
  owner / px_block    which workgroup of the streaming kernels reads element i, and pm2_*'s blocks of kPxBlock pixels
  threshold_branch    the branch of pm_threshold a pair of wet counts takes

Two things the model has to assume.  static_cast<unsigned>(NaN) is 0, which is what the hardware conversion gives:
it decides the bucket only when (v - z) * scale is inf * 0 (case range_overflow), and the device test of that case
accepts a decline as well.  And a workgroup's threads insert into the table in no fixed order, while the model inserts
in element order: which buckets find no room can depend on the order when probe sequences of different homes overlap.
hash_overflow_64x64 is built so that it cannot (one home, more buckets than probes, every bucket in every workgroup);
for hash_overflow_natural the model's count is one possible outcome.

A case is a deterministic (initial, target, claims); tests/test_probmatch_cases_cpu.py proves every claim under the
model, tests/test_probmatch_paths_gpu.py runs the cases through the three entry routes.  Most cases use min = 0 and
max = 2^20 in both arrays, so that scale is exactly 1: the target's bucket is floor(v), the initial array's floor(2 v).
"""

import functools
import os
import re
from collections import namedtuple

import numpy as np

from oracle import probmatch as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SOURCE = os.path.join(ROOT, "pysteps_amd", "csrc", "probmatch.hip")

# mirrored from probmatch.hip (tests/test_probmatch_cases_cpu.py compares them with the source text)
kBins = 1 << 20
kBinsI = 1 << 21
kSmallBin = 256
kLargeLimit = 16384
kHashBits = 12
kProbes = 8
kThreads = 256
kLoads = 4
kGrid = 2048
kPxBlock = 8192
kScanChunk = 4096
kFineBits = 12
MIRRORED = ("kBins", "kBinsI", "kSmallBin", "kLargeLimit", "kHashBits", "kProbes", "kThreads", "kLoads", "kGrid", "kPxBlock",
            "kScanChunk", "kFineBits")
kHashSlots = 1 << kHashBits
TOP = float(kBins)  # with min = 0 and max = TOP the scale is exactly 1


def parse_constants(text=None):
    """The values of the ``constexpr`` integers of probmatch.hip, evaluated from the source text."""
    if text is None:
        with open(SOURCE) as fh:
            text = fh.read()
    exprs = {}
    for line in text.splitlines():
        m = re.match(r"constexpr\s+(?:unsigned|int|size_t)\s+([^;]*);", line)  # file scope only: the kernels' own start indented
        if not m:
            continue
        for part in m.group(1).split(","):
            name, _, expr = part.partition("=")
            assert name.strip() not in exprs, "two definitions of " + name.strip()
            exprs[name.strip()] = re.sub(r"\b(0x[0-9a-fA-F]+|\d+)u\b", r"\1", expr.strip())

    def value(name, depth=0):
        assert depth < 8 and name in exprs, name
        expr = re.sub(r"\bk[A-Z]\w*", lambda mm: str(value(mm.group(0), depth + 1)), exprs[name])
        assert re.fullmatch(r"[\s\dxa-fA-F<>*/+\-()]+", expr), (name, expr)
        return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))  # integers, shifts and products only

    return {name: value(name) for name in exprs}


# ---- the model ----------------------------------------------------------------------------------------------------------
def zero_and_scale(values):
    """(z, scale) as pm_prepare fixes them: z = nanmin, scale = kBins / (max - min), 0 if max is not above min."""
    flat = np.asarray(values, np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        z, top = np.nanmin(flat), np.nanmax(flat)
        scale = np.float64(kBins) / (top - z) if top > z else np.float64(0.0)
    return np.float64(z), np.float64(scale)


def _bucket(v, z, scale, nb):
    with np.errstate(all="ignore"):
        f = (np.asarray(v, np.float64) - z) * scale
    low = np.where(np.isnan(f) | (f >= nb - 1), 0.0, f)  # NaN converts to 0; the clamped ones are replaced below
    return np.where(f >= nb - 1, nb - 1, low.astype(np.int64)).astype(np.int64)


def bin_of(v, z, scale):
    """Bucket of a wet value of the target (probmatch.hip bin_of)."""
    return _bucket(v, z, scale, kBins)


def bin_i(v, z, scale):
    """Bucket of a wet value of the initial array (bin_i): coarse = bucket >> kFineBits, fine = bucket & (2^kFineBits - 1)."""
    with np.errstate(all="ignore"):
        return _bucket(v, z, scale * np.float64(kBinsI // kBins), kBinsI)


def buckets(values, side):
    """Buckets of the wet values (> minimum; NaNs are not wet) of one array, side "initial" or "target"."""
    flat = np.asarray(values, np.float64).reshape(-1)
    z, scale = zero_and_scale(flat)
    with np.errstate(invalid="ignore"):
        wet = flat[flat > z]
    return (bin_i if side == "initial" else bin_of)(wet, z, scale)


def populations(values, side):
    """Sizes of the occupied buckets of one array, largest first (two entries at least: zeros where no bucket is)."""
    _, counts = np.unique(buckets(values, side), return_counts=True)
    return np.concatenate([np.sort(counts)[::-1], [0, 0]])


def hash_home(bucket):
    return ((np.asarray(bucket, np.int64) * 2654435761) & 0xFFFFFFFF) >> (32 - kHashBits)


def stream_grid(n):
    """Workgroups of the streaming kernels (pm_stats, pm_hist_target, pm_scatter_target, ...)."""
    return min(kGrid, (n + kLoads * kThreads - 1) // (kLoads * kThreads))


def owner(i, n):
    """The workgroup of the streaming kernels that reads element i of n."""
    return (np.asarray(i) // kThreads) % stream_grid(n)


def px_block(i):
    """The workgroup of pm2_count / pm2_scatter that owns pixel i."""
    return np.asarray(i) // kPxBlock


def table_insert(tags, bucket):
    """hash_insert: the slot of ``bucket`` in one workgroup's table (``tags``: slot -> bucket + 1, 0 free), -1 without room."""
    home = int(hash_home(bucket))
    for p in range(kProbes):
        s = (home + p) & (kHashSlots - 1)
        if tags[s] == 0 or tags[s] == bucket + 1:
            tags[s] = bucket + 1
            return s
    return -1


def table_overflow(target, workgroups=64):
    """For each of the first ``workgroups`` workgroups of pm_hist_target: the buckets of its values that find no room in
    its table, inserting in element order.  pm_scatter_target must find "no room" for exactly these again."""
    flat = np.asarray(target, np.float64).reshape(-1)
    z, scale = zero_and_scale(flat)
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero(flat > z)
    own = owner(idx, flat.size)
    b = bin_of(flat[idx], z, scale)
    order = np.argsort(own, kind="stable")
    own, b = own[order], b[order]
    edges = np.searchsorted(own, np.arange(min(stream_grid(flat.size), workgroups) + 1))
    lost = []
    for g in range(edges.size - 1):
        mine = b[edges[g]:edges[g + 1]]
        _, first = np.unique(mine, return_index=True)
        tags = np.zeros(kHashSlots, np.int64)
        lost.append([int(x) for x in mine[np.sort(first)] if table_insert(tags, int(x)) < 0])
    return lost


BRANCHES = ("fewer_wet_in_target", "equal_wet", "virt_ge_last", "t_hi", "t_lo")
EDGES = ("first_wet", "interior")


def threshold_branch(n, wet_initial, wet_target):
    """The path of pm_threshold for these counts: (branch, edge).  branch: no adjustment because the target has fewer
    ("fewer_wet_in_target") or as many ("equal_wet") wet values, ``virt >= last`` (no wet pixel in the initial array),
    or the interpolation with t >= 0.5 / t < 0.5.  edge says where the lower index ia lies: on the first wet value
    of the target, next to its block of zeros ("first_wet"), or further up ("interior").

    ia can never lie INSIDE the block of zeros, so the kernel's ``ia < zeros_trg`` selects are dead for every input:
    the adjustment needs wet_target > wet_initial, virt = (n - 1) * (1 - wi / n) = (n - wi) - (n - wi) / n lies at least
    1 / n above n - wi - 1, and n - wi - 1 >= n - wet_target = zeros_trg.  tests/test_probmatch_cases_cpu.py checks this
    exhaustively for every n up to 64."""
    if wet_target < wet_initial:
        return "fewer_wet_in_target", None
    if wet_target == wet_initial:
        return "equal_wet", None
    war = np.float64(wet_initial) / np.float64(n)
    q = (100.0 * (1.0 - war)) / 100.0
    last = np.float64(n - 1)
    virt = last * q
    zeros_trg = n - wet_target
    if virt >= last:
        return "virt_ge_last", "first_wet" if n - 1 == zeros_trg else "interior"
    fl = np.floor(virt)
    ia = int(fl)
    edge = "inside_zeros" if ia < zeros_trg else ("first_wet" if ia == zeros_trg else "interior")
    return ("t_hi" if virt - fl >= 0.5 else "t_lo"), edge


# ---- the cases -----------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name initial target claims")
# claims: a dict the CPU test checks under the model.  Keys used:
#   declined      the kernels answer PSH_EUNSUPPORTED (absent: handled)
#   ties          the initial array has tied wet values (the reference is then compared per tie group)
#   degenerate    a decline is acceptable on the device, a different field is not
#   largest       {"side": (largest bucket, second largest bucket)} of the wet values
#   equal_run     {"side": number of equal wet values}
#   overflow      (workgroups with overflow, overflowed buckets in all) over the first 64 workgroups
#   anything else is explained where it is set

_BUILDERS = {}
_OUTCOME = {}  # name -> "handled", "declined" or "degenerate", known without building the arrays


def _case(name, outcome="handled"):
    def register(fn):
        assert name not in _BUILDERS, name
        _BUILDERS[name] = fn
        _OUTCOME[name] = outcome
        return fn
    return register


def names():
    return list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def get(name):
    initial, target, claims = _BUILDERS[name]()
    initial = np.ascontiguousarray(initial, np.float64)
    target = np.ascontiguousarray(target, np.float64)
    assert initial.shape == target.shape and initial.ndim == 1
    initial.setflags(write=False)
    target.setflags(write=False)
    return Case(name, initial, target, claims)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's field of a case, computed once and shared."""
    case = get(name)
    with np.errstate(all="ignore"):
        out = oracle.nonparam_match_empirical_cdf(case.initial, case.target)
    out.setflags(write=False)
    return out


def _rng(name):
    return np.random.default_rng([ord(ch) for ch in name])


def _ramp(rng, n):
    """A tie-free permutation of 0 .. n-1: one value per bucket on either side as long as n <= 2^20."""
    return rng.permutation(n).astype(np.float64)


def _lonely(count, first=1000):
    """``count`` values between 0 and TOP, each alone in its bucket on either side: j + 0.25 for consecutive j."""
    assert first + count < kBins - 1
    return np.arange(first, first + count, dtype=np.float64) + 0.25


def _framed(rng, body):
    """``body`` with the minimum 0 and the maximum TOP added (scale exactly 1), shuffled."""
    out = np.concatenate([[0.0, TOP], body])
    rng.shuffle(out)
    return out


# the per-workgroup bucket table
HASH_BUCKETS = 40


def hash_family():
    """Buckets that share the hash home of the last bucket (the maximum's own, so that every wet value of the target can
    come from the family), the last bucket first."""
    family = np.flatnonzero(hash_home(np.arange(kBins)) == hash_home(kBins - 1))
    return np.concatenate([[kBins - 1], family[family != kBins - 1]])


@_case("hash_overflow_64x64")
def _hash_overflow_small():
    rng = _rng("hash_overflow_64x64")
    n = 64 * 64
    family = hash_family()[:HASH_BUCKETS]
    values = np.where(family == kBins - 1, TOP, family + 0.5)  # the maximum is clamped into the last bucket
    target = values[rng.integers(0, HASH_BUCKETS, n)]
    target[rng.random(n) < 0.3] = 0.0
    return _ramp(rng, n), target, {"overflow": (4, 4 * (HASH_BUCKETS - kProbes)), "one_home": True}


NATURAL_STEP = 256
NATURAL_SHARE = 0.25
NATURAL_SIDE = 1792  # the smallest side that passes (63 of the first 64 workgroups; 1536 has 14 of 64); tests/test_probmatch_cases_cpu.py


def natural_target(side):
    return np.random.default_rng(side).standard_normal(side * side)


def natural_share(side, workgroups=64):
    """(share of the first ``workgroups`` workgroups with overflow, overflowed buckets in them)"""
    lost = table_overflow(natural_target(side), workgroups)
    return sum(1 for x in lost if x) / len(lost), sum(len(x) for x in lost)


@_case("hash_overflow_natural")
def _hash_overflow_natural():
    n = NATURAL_SIDE * NATURAL_SIDE
    initial = np.random.default_rng(NATURAL_SIDE + 1).standard_normal(n)
    return initial, natural_target(NATURAL_SIDE), {"natural": True}


# bucket populations around kSmallBin and kLargeLimit
BUCKET_COUNTS = (kSmallBin - 1, kSmallBin, kSmallBin + 1, kLargeLimit - 1, kLargeLimit, kLargeLimit + 1)


def _crowd(c):
    """c unequal values in bucket 100 of the target and bucket 200 of the initial array."""
    assert c < 1 << 15  # below 100.5: one bucket on either side
    return 100.0 + np.arange(c, dtype=np.float64) * 2.0 ** -16


def _bucket_case(c, side):
    name = "bucket_%d_%s" % (c, side)

    def build():
        rng = _rng(name)
        n = max(4096, 2 * c)
        crowded = _framed(rng, np.concatenate([_crowd(c), _lonely(n - c - 2)]))
        other = _ramp(rng, n)
        claims = {"largest": {side: (c, 1)}}
        if c > kLargeLimit:
            claims["declined"] = True
        return (crowded, other, claims) if side == "initial" else (other, crowded, claims)
    _case(name, "declined" if c > kLargeLimit else "handled")(build)


for _c in BUCKET_COUNTS:
    for _side in ("initial", "target"):
        _bucket_case(_c, _side)


def _tied_case(c):
    name = "tied_%d_initial" % c

    def build():
        rng = _rng(name)
        n = max(4096, 2 * c)
        initial = _framed(rng, np.concatenate([np.full(c, 100.0), _lonely(n - c - 2)]))
        claims = {"largest": {"initial": (c, 1)}, "equal_run": {"initial": c}, "ties": True}
        if c > kLargeLimit:
            claims["declined"] = True
        return initial, _ramp(rng, n), claims
    _case(name, "declined" if c > kLargeLimit else "handled")(build)


for _c in (kLargeLimit, kLargeLimit + 1):
    _tied_case(_c)


@_case("equal_40000_target")
def _equal_target():
    rng = _rng("equal_40000_target")
    c, n = 40000, 80000
    target = _framed(rng, np.concatenate([np.full(c, 100.0), _lonely(n - c - 2)]))
    return _ramp(rng, n), target, {"largest": {"target": (c, 1)}, "equal_run": {"target": c}}  # mn == mx: never declined


# every pair of wet counts of tiny arrays: the branches of pm_threshold
SMALL_N = tuple(range(1, 10))


def wet_count_pairs(n, with_nan):
    """(initial, target, (wet_initial, wet_target)) for every pair of wet counts in 0 .. n-1, distinct wet values; with_nan:
    one of the target's zeros is a NaN instead (only where another zero remains to be the minimum)."""
    rng = _rng("wet_counts_n%d_%d" % (n, with_nan))
    out = []
    for wi in range(n):
        for wt in range(n):
            if with_nan and n - wt < 2:
                continue
            initial = np.concatenate([np.full(n - wi, -15.0), -15.0 + np.cumsum(rng.uniform(0.5, 2.0, wi))])
            target = np.concatenate([np.full(n - wt, 0.25), 0.25 + np.cumsum(rng.uniform(0.1, 3.0, wt))])
            if with_nan:
                target[0] = np.nan
            out.append((rng.permutation(initial), rng.permutation(target), (wi, wt)))
    return out


# degenerate bucket scales
@_case("range_overflow", "degenerate")
def _range_overflow():
    rng = _rng("range_overflow")
    draw = lambda: (rng.random(5000) * 2.0 - 1.0) * 1.7e308
    return draw(), draw(), {"degenerate": True, "scale": 0.0}


@_case("range_denormal", "degenerate")
def _range_denormal():
    rng = _rng("range_denormal")
    return _ramp(rng, 5000) * 5e-324, _ramp(rng, 5000) * 5e-324, {"degenerate": True, "scale": np.inf}


ULP_PAIRS = 600


def ulp_pairs():
    """(lower, upper) values one ulp apart, and whether they share a bucket on (target, initial) side: inside a bucket, across
    an edge of both sides' buckets (an integer) and across an edge of the initial array's alone (a half)."""
    lo, hi, same = [], [], []
    for j in range(ULP_PAIRS):
        base = 1000.0 + 3 * j
        for upper, shared in ((np.nextafter(base + 0.25, TOP), (True, True)), (base + 1.0, (False, False)), (base + 1.5, (True, False))):
            lo.append(np.nextafter(upper, 0.0))
            hi.append(upper)
            same.append(shared)
    return np.array(lo), np.array(hi), same


@_case("ulp_neighbours")
def _ulp_neighbours():
    rng = _rng("ulp_neighbours")
    lo, hi, _ = ulp_pairs()
    body = np.concatenate([lo, hi])
    return _framed(rng, body), _framed(rng, body), {"ulp": True}


@_case("signed_zero_minimum")
def _signed_zero():
    rng = _rng("signed_zero_minimum")
    n = 4096
    zeros = np.where(np.arange(1500) % 2 == 0, 0.0, -0.0)
    initial = rng.permutation(np.concatenate([zeros, _lonely(n - 1500 - 1), [TOP]]))
    target = rng.permutation(np.concatenate([-zeros[:1200], _lonely(n - 1200 - 1), [TOP]]))
    return initial, target, {"signed_zeros": True}


# sizes: the edges of kThreads, kLoads * kThreads, kPxBlock (and the ragged last chunk of pm2_offsets: kScanChunk entries of H)
SIZES = (1, 2, kThreads - 1, kThreads, kThreads + 1, kLoads * kThreads - 1, kLoads * kThreads, kLoads * kThreads + 1,
         kPxBlock - 1, kPxBlock, kPxBlock + 1, 8 * kPxBlock - 1, 8 * kPxBlock, 8 * kPxBlock + 1)


def _size_case(n, quantised):
    name = "size_%d%s" % (n, "_quantised" if quantised else "")

    def build():
        rng = _rng(name)
        initial = rng.normal(size=n) * 5
        target = rng.normal(size=n) * 6
        if quantised:
            target = np.round(target, 1)
            target[target < -3.0] = -15.0
        return initial, target, {"tie_free_initial": True}
    _case(name)(build)


for _n in SIZES:
    _size_case(_n, False)
    _size_case(_n, True)


# two probes that separate the halves of the work
PROBE_N = 70 * 90


@_case("probe_sorted_target")
def _probe_sorted_target():
    """out[pixel whose initial value is k] is the k-th smallest target value (NaNs as the minimum): holds tw in full."""
    rng = _rng("probe_sorted_target")
    target = np.round(rng.normal(size=PROBE_N) * 6, 1)
    target[target < -2.0] = -15.0
    target[rng.random(PROBE_N) < 0.05] = np.nan
    return _ramp(rng, PROBE_N), target, {"probe": "target"}


@_case("probe_initial_ranks")
def _probe_initial_ranks():
    """The target is a shuffled ramp: out is the stable rank of every wet pixel of the initial array, 0 on the dry ones."""
    rng = _rng("probe_initial_ranks")
    initial = np.round(rng.normal(size=PROBE_N) * 4, 1)  # tie groups
    initial[initial < -1.0] = -15.0  # a dry block
    return initial, _ramp(rng, PROBE_N), {"probe": "initial", "ties": True}


def probe_expected(case):
    """What the probe's identity says the output is, without the oracle."""
    if case.claims["probe"] == "target":
        ranked = np.sort(np.where(np.isnan(case.target), np.nanmin(case.target), case.target))
        return ranked[case.initial.astype(np.int64)]
    order = np.argsort(case.initial, kind="stable")
    ranks = np.empty(case.initial.size, np.float64)
    ranks[order] = np.arange(case.initial.size)
    return np.where(case.initial > case.initial.min(), ranks, 0.0)


def with_outcome(outcome):
    return [n for n in names() if _OUTCOME[n] == outcome]
