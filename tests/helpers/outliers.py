"""Exact yardstick and case generator for the local outlier test of sparse vectors (test infrastructure).

``pysteps/utils/cleansing.py`` ``detect_outliers`` (local, multivariate form): for every vector the k nearest OTHER
vectors, ``z = uv - mean(neighbours)``, ``C = cov(neighbours, ddof=1)``, outlier iff ``sqrt(z^T C^-1 z) > thr``; a
singular ``C`` is not an outlier.  The HIP kernels (``csrc/sparse_qc.hip``) document which neighbours they take:

* the key of candidate ``j`` of vector ``i`` is ``(float32(dx*dx + dy*dy), j)`` with ``dx``, ``dy`` and the sum in
  float64, ascending; the first ``kk = min(n, k + 1)`` candidates are extracted;
* the first of them is dropped - the vector itself, or a vector at the same position with a lower index.

``knn_by_key`` is that rule in NumPy (a stable sort of the float32 values), ``knn_by_float64`` the same with the
unrounded float64 squared distance; the second only shows where the two rules part.

``verdict`` evaluates the test on a neighbour set in ``np.longdouble`` with the two-pass mean and covariance.  The
covariance is singular when

* fewer than three neighbours are left: the sample covariance of ``cnt`` points has rank ``<= cnt - 1``, so two
  neighbours span a line at most and ``det`` is 0 in exact arithmetic.  What a floating-point ``det`` returns there is
  the rounding residue of ``caa*cbb - cab*cab``, of either sign - no verdict can be held to it;
* or the longdouble determinant is exactly 0 (the collinear constructions below: ``v = u``, ``v = 2u``, ``v = -u``
  scale ``caa``, ``cab``, ``cbb`` by exact powers of two, both products round alike).

``margin`` is a condition on the INPUTS, not a tolerance on the kernel: ``min |md - thr| / thr`` over the vectors.  A
float64 one-pass kernel cannot be held to a verdict that sits on the threshold, so every case must have
``margin >= MIN_MARGIN`` under the longdouble oracle alone, and ``onepass_float64`` (the kernel's formulas in plain
float64, no FMA) must reproduce the longdouble ``md`` to ``MAX_FORMULA_DEV`` relative: the verdict is then a factor
1000 away from the formula's own error.  ``fragile_keys`` is the analogous condition on the ordering key: a compiler
may or may not fuse ``dx*dx + dy*dy`` into one FMA, which moves the float64 sum by an ulp; no candidate whose float32
key sits within one float32 step of the kk-th key may change its float32 rounding under that ulp.
"""

import functools

import numpy as np

THR = 3.0
MIN_MARGIN = 1e-6
MAX_FORMULA_DEV = 1e-9
MIN_NEIGHBOURS = 3  # fewer neighbours than this: rank-deficient covariance, never an outlier
SAMPLE_ABOVE = 2100  # above this many vectors the yardstick is evaluated on SAMPLE_ROWS rows + the fixed ones
SAMPLE_ROWS = 512
MAX_N = 8192  # csrc/sparse_qc.hip kQcMaxN


def kernel_of(n):
    """The kernel ``launch_outliers`` picks for ``n`` rows."""
    return "sorted16" if n <= 1024 else "sorted32" if n <= 2048 else "rescan"


# ---- neighbour sets ----------------------------------------------------------------------------------------------
def _d2(xy, rows):
    """(R, n) float64 ``dx*dx + dy*dy`` of the float64 differences, every operation rounded (no FMA)."""
    dx = xy[None, :, 0] - xy[rows, None, 0]
    dy = xy[None, :, 1] - xy[rows, None, 1]
    return dx * dx + dy * dy


def _chunks(rows, n):
    step = max(1, (1 << 21) // max(n, 1))
    for s in range(0, len(rows), step):
        yield rows[s:s + step]


def _select(xy, k, rows, dtype, extra=0, higher_index_first=False):
    xy = np.asarray(xy, np.float64)
    n = xy.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    kk = min(n, k + 1)
    take = min(n, kk + extra)
    order = np.empty((len(rows), take), np.int64)
    keys = np.empty((len(rows), take), dtype)
    at = 0
    for r in _chunks(rows, n):
        key = _d2(xy, r).astype(dtype)
        if higher_index_first:  # the wrong rule, for mistaken_flags only
            o = n - 1 - np.argsort(key[:, ::-1], axis=1, kind="stable")[:, :take]
        else:
            o = np.argsort(key, axis=1, kind="stable")[:, :take]  # stable: equal keys stay in index order
        order[at:at + len(r)] = o
        keys[at:at + len(r)] = np.take_along_axis(key, o, axis=1)
        at += len(r)
    return order, keys, kk


def knn_by_key(xy, k, rows=None):
    """(R, kk - 1) neighbour indices in extraction order under the kernel's rule (float32 key, then index)."""
    order, _, kk = _select(xy, k, rows, np.float32)
    return order[:, 1:kk]


def knn_by_float64(xy, k, rows=None):
    """The same with the float64 squared distance as the key."""
    order, _, kk = _select(xy, k, rows, np.float64)
    return order[:, 1:kk]


def tie_rows(xy, k, rows=None):
    """bool (R,): the kk-th and the (kk+1)-th candidate carry the same float32 key (the index decides)."""
    _, keys, kk = _select(xy, k, rows, np.float32, extra=1)
    if keys.shape[1] <= kk:
        return np.zeros(keys.shape[0], bool)
    return keys[:, kk - 1] == keys[:, kk]


def fragile_keys(xy, k, rows=None):
    """Number of candidates whose float32 key is within one float32 step of the kk-th key AND would round to another
    float32 if the float64 sum moved by one ulp (fused or unfused ``dx*dx + dy*dy``)."""
    xy = np.asarray(xy, np.float64)
    n = xy.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    kk = min(n, k + 1)
    if kk >= n:
        return 0  # every key is extracted: the order inside the set does not matter
    bad = 0
    for r in _chunks(rows, n):
        d2 = _d2(xy, r)
        bits = d2.astype(np.float32).view(np.uint32).astype(np.int64)
        kth = np.partition(bits, kk - 1, axis=1)[:, kk - 1:kk]
        near = np.abs(bits - kth) <= 1
        lo = np.nextafter(d2, -np.inf).astype(np.float32)
        hi = np.nextafter(d2, np.inf).astype(np.float32)
        bad += int(np.count_nonzero(near & (lo != hi)))
    return bad


# ---- verdicts ----------------------------------------------------------------------------------------------------
def verdict(uv, nb, rows, thr=THR):
    """(md, singular) in longdouble for the vectors ``rows`` with the neighbours ``nb`` (R, cnt)."""
    L = np.longdouble
    uv = np.asarray(uv, np.float64)
    rows = np.asarray(rows, np.int64)
    cnt = nb.shape[1]
    md = np.zeros(len(rows), L)
    singular = np.ones(len(rows), bool)
    if cnt < MIN_NEIGHBOURS:
        return md, singular
    step = max(1, (1 << 18) // cnt)
    for s in range(0, len(rows), step):
        e = min(len(rows), s + step)
        nbv = uv[nb[s:e]].astype(L)  # (r, cnt, 2)
        mean = nbv.sum(axis=1) / L(cnt)
        dev = nbv - mean[:, None, :]
        z = uv[rows[s:e]].astype(L) - mean
        dof = L(cnt - 1)
        caa = (dev[..., 0] * dev[..., 0]).sum(axis=1) / dof
        cab = (dev[..., 0] * dev[..., 1]).sum(axis=1) / dof
        cbb = (dev[..., 1] * dev[..., 1]).sum(axis=1) / dof
        det = caa * cbb - cab * cab
        ok = det != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            md2 = (z[:, 0] * z[:, 0] * cbb - L(2) * z[:, 0] * z[:, 1] * cab + z[:, 1] * z[:, 1] * caa) / det
        assert np.all(md2[ok] >= 0), "negative squared distance in the longdouble yardstick"
        md[s:e][ok] = np.sqrt(md2[ok])
        singular[s:e] = ~ok
    return md, singular


def onepass_float64(uv, nb, rows):
    """(md, singular): the kernel's own formulas in plain float64, products rounded before they are added - sums of
    the neighbours relative to the vector itself, in extraction order, one pass."""
    uv = np.asarray(uv, np.float64)
    rows = np.asarray(rows, np.int64)
    cnt = nb.shape[1]
    md = np.zeros(len(rows))
    singular = np.ones(len(rows), bool)
    if cnt < MIN_NEIGHBOURS:
        return md, singular
    step = max(1, (1 << 18) // cnt)
    for s in range(0, len(rows), step):
        e = min(len(rows), s + step)
        rel = uv[nb[s:e]] - uv[rows[s:e]][:, None, :]
        a, b = rel[..., 0], rel[..., 1]
        # cumsum adds one term after the other, like the kernel's loop (sum() would add pairwise)
        sa, sb = np.cumsum(a, axis=1)[:, -1], np.cumsum(b, axis=1)[:, -1]
        saa, sab, sbb = (np.cumsum(p, axis=1)[:, -1] for p in (a * a, a * b, b * b))
        ma, mb = sa / cnt, sb / cnt
        dof = float(cnt - 1)
        t1, t2, t3 = sa * ma, sa * mb, sb * mb
        caa, cab, cbb = (saa - t1) / dof, (sab - t2) / dof, (sbb - t3) / dof
        p1, p2 = caa * cbb, cab * cab
        det = p1 - p2
        ok = (det != 0) & np.isfinite(det)
        zu, zv = -ma, -mb
        q1, q2, q3 = zu * zu * cbb, 2.0 * zu * zv * cab, zv * zv * caa
        with np.errstate(divide="ignore", invalid="ignore"):
            md2 = ((q1 - q2) + q3) / det
            md[s:e] = np.where(ok, np.sqrt(md2), 0.0)
        singular[s:e] = ~ok
    return md, singular


def oracle_flags(xy, uv, k, thr=THR, rows=None):
    """bool flags of ``rows`` (all by default) for any input: the kernel's neighbour rule, the longdouble verdict."""
    xy = np.asarray(xy, np.float64)
    rows = np.arange(xy.shape[0]) if rows is None else np.asarray(rows, np.int64)
    if xy.shape[0] < 2:
        return np.zeros(len(rows), bool)
    md, singular = verdict(uv, knn_by_key(xy, k, rows), rows, thr)
    return np.asarray(md > thr) & ~singular


def sample_rows(n):
    """All rows up to SAMPLE_ABOVE vectors; beyond, a fixed random sample plus the first row, the rows around the first
    wave-sized block and the last one (the device computes every row all the same)."""
    if n <= SAMPLE_ABOVE:
        return np.arange(n)
    pick = np.random.default_rng(n).choice(n, SAMPLE_ROWS, replace=False)
    return np.unique(np.concatenate([pick, [0, 63, 64, n - 1]]))


class Expected:
    """What the yardstick says about one case: the rows it looked at, their flags, and the input conditions."""

    def __init__(self, case, selector=knn_by_key):
        self.rows = rows = sample_rows(case.n)
        self.nb = nb = selector(case.xy, case.k, rows)
        self.md, self.singular = verdict(case.uv, nb, rows, case.thr)
        self.flags = np.asarray(self.md > case.thr) & ~self.singular
        self.margin = float(np.min(np.abs(self.md - case.thr) / case.thr)) if len(rows) else 1.0
        md64, sing64 = onepass_float64(case.uv, nb, rows)
        self.singular_agrees = bool(np.array_equal(sing64, self.singular))
        ok = ~self.singular & ~sing64
        with np.errstate(divide="ignore", invalid="ignore"):
            dev = np.abs(md64[ok] - self.md[ok]) / self.md[ok]
        self.formula_dev = float(dev.max()) if dev.size else 0.0
        self.flags64 = np.asarray(md64 > case.thr) & ~sing64


MISTAKES = ("second_chunk", "higher_index", "last_vector_missing", "float64_key")


def mistaken_flags(case, mistake):
    """(rows, flags) the yardstick gives when ONE rule of the kernels is deliberately broken - only to show that a
    case can tell (tests/test_outliers_cpu.py asserts that the flags then differ from the right ones):

    * ``second_chunk``: the first key of every later chunk of 64 extractions is dropped like the very first one;
    * ``higher_index``: equal float32 keys go to the higher index;
    * ``last_vector_missing``: vector n - 1 is no candidate (a kernel that holds 64 x KPER keys given one row more);
    * ``float64_key``: the unrounded squared distance orders the candidates.
    """
    rows = sample_rows(case.n)
    xy, uv = case.xy, case.uv
    if mistake == "last_vector_missing":
        rows, xy, uv = rows[rows != case.n - 1], xy[:-1], uv[:-1]
    if mistake == "float64_key":
        nb = knn_by_float64(xy, case.k, rows)
    else:
        order, _, kk = _select(xy, case.k, rows, np.float32, higher_index_first=mistake == "higher_index")
        nb = order[:, 1:kk]
    if mistake == "second_chunk":
        nb = np.delete(nb, [t0 - 1 for t0 in range(64, nb.shape[1] + 1, 64)], axis=1)
    md, singular = verdict(uv, nb, rows, case.thr)
    return rows, np.asarray(md > case.thr) & ~singular


# ---- cases -------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, xy, uv, k, thr=THR, kind="continuous"):
        self.name, self.k, self.thr, self.kind = name, int(k), float(thr), kind
        self.xy = np.ascontiguousarray(xy, np.float64)
        self.uv = np.ascontiguousarray(uv, np.float64)
        self.n = self.xy.shape[0]
        assert self.xy.shape == (self.n, 2) and self.uv.shape == (self.n, 2)
        self.kernel = kernel_of(self.n)
        self.id = "%s-%s" % (self.kernel, name)

    @property
    def tie_free(self):
        return self.kind in ("continuous", "k_ge_n", "large", "collinear")


def _vectors(rng, n):
    """N(0, 1) + (3, -2) with about n / 30 planted outliers."""
    uv = rng.normal(0, 1, (n, 2)) + [3, -2]
    bad = rng.choice(n, max(1, n // 30), replace=False)
    uv[bad] += rng.choice([-1.0, 1.0], (bad.size, 2)) * rng.uniform(4, 9, (bad.size, 2))
    return uv


def _continuous(name, n, k, seed, kind="continuous"):
    rng = np.random.default_rng(seed)
    return Case(name, rng.uniform(0, 4096, (n, 2)), _vectors(rng, n), k, kind=kind)


def _lattice(name, n, k, side, seed):
    """Integer positions in [0, side)^2 (side^2 * 2 < 2^24: every squared distance exact in float32), 8 % of them
    moved onto another vector's position."""
    assert 2 * (side - 1) ** 2 < 2 ** 24
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, side, (n, 2)).astype(np.float64)
    dup = rng.choice(n, int(np.ceil(0.08 * n)), replace=False)
    keep = np.setdiff1d(np.arange(n), dup)
    xy[dup] = xy[rng.choice(keep, dup.size)]
    return Case(name, xy, _vectors(rng, n), k, kind="lattice")


NEAR_TIE_MIN = 20


def near_tie_rows(case):
    """Rows of ``case`` whose kk-th and (kk+1)-th candidates BY FLOAT64 DISTANCE differ by a relative 1e-9 .. 1e-8,
    share one float32 key, and have the closer one at the higher index."""
    order, keys, kk = _select(case.xy, case.k, None, np.float64, extra=1)
    near, far = keys[:, kk - 1], keys[:, kk]
    gap = (far - near) / near
    same32 = near.astype(np.float32) == far.astype(np.float32)
    return np.flatnonzero((gap >= 1e-9) & (gap <= 1e-8) & same32 & (order[:, kk - 1] > order[:, kk]))


def _put_between(uv, c, set_a, set_b):
    """Moves the vector of ``c`` along u to where the threshold lies halfway between the Mahalanobis distances it has
    with the neighbours ``set_a`` and with the neighbours ``set_b``: which set is taken decides its flag."""
    sets = [np.asarray(s, np.int64)[None, :] for s in (set_a, set_b)]
    centre = uv[np.intersect1d(set_a, set_b)].mean(axis=0)

    def total(alpha):
        uv[c] = centre + [alpha, 0.0]
        return sum(float(verdict(uv, nb, [c])[0][0]) for nb in sets)

    lo, hi = 0.0, 64.0  # from a few sigma on, both distances grow with alpha
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if total(mid) < 2 * THR else (lo, mid)
    total(hi)


def _last_matters(name, n, k, seed):
    """Continuous positions; the LAST vector deviates by (5, 5), and the vector nearest to it has its flag decided by
    whether the last one is among its neighbours or the (kk+1)-th candidate takes its place - what a kernel that
    holds n - 1 keys would do."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 4096, (n, 2))
    uv = _vectors(rng, n)
    last = n - 1
    uv[last] = [8.0, 3.0]
    kk = min(n, k + 1)
    c = int(np.argsort(_d2(xy, np.array([last]))[0], kind="stable")[1])
    o = np.argsort(_d2(xy, np.array([c]))[0], kind="stable")
    assert last in o[1:kk]
    _put_between(uv, c, o[1:kk], [j for j in o[1:kk + 1] if j != last])
    return Case(name, xy, uv, k, kind="continuous")


def _near_ties(name, n, k, seed):
    """Continuous positions; for some thirty vectors c the (kk+1)-th candidate is then pulled along its ray until its
    float64 squared distance is a relative 3e-9 away from the kk-th one's - on the far side if its index is the lower
    one, on the near side otherwise, so that the closer of the two always carries the higher index.  The vector of c
    is then put where the threshold lies halfway between the Mahalanobis distances it has with either of the two
    among its neighbours: which one is taken decides its flag.  The neighbourhoods of these vectors do not overlap."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 4096, (n, 2))
    uv = _vectors(rng, n)
    kk = min(n, k + 1)
    touched = set()
    done = 0
    for c in rng.permutation(n):
        c = int(c)
        d2 = _d2(xy, np.array([c]))[0]
        o = np.argsort(d2, kind="stable")
        a, b = int(o[kk - 1]), int(o[kk])
        if set(o[:kk + 1].tolist()) & touched:
            continue
        target = d2[a] * (1 + 3e-9) if b < a else d2[a] * (1 - 3e-9)
        xy[b] = xy[c] + (xy[b] - xy[c]) * np.sqrt(target / d2[b])
        _put_between(uv, c, o[1:kk], np.append(o[1:kk - 1], b))
        touched |= set(o[:kk + 1].tolist())
        done += 1
        if done == 30:
            break
    return Case(name, xy, uv, k, kind="near_tie")


def _collinear(name, n, k, how, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 4096, (n, 2))
    u = rng.normal(0, 1, n) + 3
    if how == "same":
        uv = np.tile([3.0, -2.0], (n, 1))
    else:
        v = {"v=u": u, "v=2u": 2 * u, "v=-u": -u, "v=0": np.zeros(n)}[how]
        uv = np.column_stack([u, v])
    return Case(name, xy, uv, k, kind="collinear")


LARGE_SHIFT = np.array([2.6e5, 9.6e5])  # projected metres


def large_base():
    """The large-coordinate case before the shift: positions on a 2^-16 grid, so that adding LARGE_SHIFT is exact
    and every float64 difference is the same number."""
    rng = np.random.default_rng(77)
    xy = np.round(rng.uniform(0, 4096, (1025, 2)) * 65536.0) / 65536.0
    return Case("large-base-n1025-k30", xy, _vectors(rng, 1025), 30, kind="large")


def _large(name):
    base = large_base()
    xy = base.xy + LARGE_SHIFT
    assert np.array_equal(xy - LARGE_SHIFT, base.xy)
    return Case(name, xy, base.uv, 30, kind="large")


def _builders():
    b = {}
    for n in (2, 3, 4, 31, 32, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 8192):
        b["cont-n%d-k30" % n] = functools.partial(_continuous, n=n, k=30, seed=1000 + n)
    for k in (1, 2, 63, 64, 65, 127, 128, 200):
        b["chunks-n700-k%d" % k] = functools.partial(_continuous, n=700, k=k, seed=2000 + k)
    for n in (1500, 2100):
        for k in (64, 129):
            b["chunks-n%d-k%d" % (n, k)] = functools.partial(_continuous, n=n, k=k, seed=3000 + n + k)
    for n, k in ((64, 100), (1024, 5000), (1100, 2000), (2049, 2049)):
        b["all-n%d-k%d" % (n, k)] = functools.partial(_continuous, n=n, k=k, seed=4000 + n, kind="k_ge_n")
    for n, side in ((900, 400), (1800, 400), (3000, 400), (8192, 2896)):
        b["lattice-n%d-k30" % n] = functools.partial(_lattice, n=n, k=30, side=side, seed=5000 + n)
    # the first row count beyond what each sorted kernel holds, with a flag that hangs on the last vector (among
    # thirty random neighbours a lost candidate rarely moves a flag)
    for n in (1025, 2049):
        b["last-n%d-k30" % n] = functools.partial(_last_matters, n=n, k=30, seed=8000 + n)
    b["neartie-n600-k8"] = functools.partial(_near_ties, n=600, k=8, seed=6000)
    b["large-n1025-k30"] = _large
    for n in (200, 1500, 2500):
        for how in ("v=u", "v=2u", "v=-u", "v=0", "same"):
            b["collinear-%s-n%d-k30" % (how, n)] = functools.partial(_collinear, n=n, k=30, how=how, seed=7000 + n)
    b["collinear-v=u-n40-k100"] = functools.partial(_collinear, n=40, k=100, how="v=u", seed=7040)
    return b


_BUILDERS = _builders()
NAMES = list(_BUILDERS)
IDS = ["%s-%s" % (kernel_of(int(nm.split("-n")[1].split("-")[0])), nm) for nm in NAMES]


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name](name=name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The yardstick of a case, computed once per process and shared (callers must not write into it)."""
    return Expected(case(name))


def recorded(name):
    """What tests/golden/outliers_margins.json keeps per case (settings and recorded results only)."""
    c, e = case(name), expected(name)
    return {"n": c.n, "k": c.k, "thr": c.thr, "kind": c.kind, "kernel": c.kernel, "rows_checked": int(len(e.rows)),
            "flagged": int(e.flags.sum()), "singular": int(e.singular.sum()), "margin": e.margin,
            "formula_dev": e.formula_dev, "tie_share": float(tie_rows(c.xy, c.k, e.rows).mean())}


if __name__ == "__main__":  # python tests/helpers/outliers.py: rewrite tests/golden/outliers_margins.json
    import json
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "outliers_margins.json")
    with open(path, "w") as f:
        json.dump({name: recorded(name) for name in NAMES}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, len(NAMES), "cases")
