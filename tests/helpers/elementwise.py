"""Plain NumPy restatement of the resident element-wise passes (csrc/elementwise.hip) and the cases they are held to.

Imports no device code.  What is restated:

* ``db_forward`` / ``db_inverse``: pysteps/utils/transformation.py:150-232.  The zero mask is a comparison and is
  exact: it is decided in the field's dtype or in float64, whichever ``np.result_type`` names for the threshold
  *object* (a Python float or int and a ``numpy.float32`` meet a float32 field in float32, a ``numpy.float64``
  scalar meets it in float64).  The promotion is written out here with ``astype`` so that it does not lean on the
  implicit rule it restates.  The values are evaluated in float64 from the float32 input; a float32 result is
  compared with them in units of the float32 spacing of the float64 value (``deviation``).
* ``stats``: the reductions ``psh_field_stats_dev`` / ``psh_count_above_dev`` return.

The bars: the unmodified reference evaluates the transcendental in float32 (``10.0 * np.log10(R)``,
``10.0 ** (R / 10.0)``), so it deviates from the float64 value itself.  ``measure`` takes that deviation over
``cases()``, per direction; tests/golden/elementwise_bars.json stores it to four significant digits and the device
is given ``BAR_FACTOR`` times it, the margin for a second correct float32 implementation of the same transcendental.
``python -m helpers.elementwise`` from tests/ rewrites the file (it needs the reference package, oracle/_ref).

The inverse decision ``10^(R/10) < threshold`` is a comparison of a *computed* float32 value, so two correct
implementations may differ where the float64 value lies within the bar of the threshold.  ``InverseExpectation.near``
marks those elements; everywhere else the decision is exact.
"""

import json
import os
import warnings

import numpy as np

BARS_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "elementwise_bars.json")
BAR_FACTOR = 5.0
NEAR_CAP = 1e-3  # largest share of a continuous case's elements that may lie within the bar of the threshold

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
FLT_MIN = float(np.finfo(F32).tiny)  # the smallest normal
SUBNORMAL = float(F32(1e-40))

SIZES = (1, 2, 3, 4, 5, 7, 1023, 4099)  # float4 body and tail
STATS_LOOP = 300_000  # > 1024 blocks x 256 threads: a field_stats thread loops
GRID_STRIDE = 2_100_003  # > 256 CUs x 8 blocks x 256 threads x 4: the dB kernel's grid stride runs, with a tail of 3
STACK_SHAPE = (3, 37, 53)  # 1961-pixel planes: views 1 and 2 start 4 and 8 bytes off 16-byte alignment
THRESHOLDS = (0.1, 0.5, 0.7, 0.03, 0.16)
FORWARD_ZERO = -1000.0  # below 10 log10 of the smallest subnormal (-450): no computed value can equal it
INVERSE_ZERO = -1.0  # 10^x is never negative


# ---- the restatement ----------------------------------------------------------------------------------------------------


def compared_with(threshold, dtype=F32):
    """The float64 number that decides ``field < threshold`` for a field of ``dtype``, as NumPy evaluates it."""
    common = np.result_type(dtype, threshold)
    with np.errstate(over="ignore"):
        return float(np.asarray(threshold).astype(common))


def less_than(field, threshold):
    """``field < threshold`` with NumPy's promotion written out."""
    common = np.result_type(field.dtype, threshold)
    with np.errstate(over="ignore"):
        return field.astype(common) < np.asarray(threshold).astype(common)


def spacing32(x64):
    """Distance from float32(|x|) to the next float32, as float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.spacing(np.abs(np.asarray(x64, dtype=np.float64)).astype(F32)).astype(np.float64)


class ForwardExpectation:
    def __init__(self, zeros, value):
        self.zeros, self.value = zeros, value  # value: float64, meaningful where ~zeros


def db_forward(R, threshold, zerovalue):
    """zeros = R < threshold; elsewhere 10 log10(R) in float64 (NaN for NaN and for negative values, -inf for +-0)."""
    del zerovalue  # the mask and the values do not depend on it; the signature is the operation's
    R = np.asarray(R)
    zeros = less_than(R, threshold)
    with np.errstate(divide="ignore", invalid="ignore"):
        value = 10.0 * np.log10(R.astype(np.float64))
    return ForwardExpectation(zeros, value)


def forward_threshold_db(threshold):
    """metadata["threshold"] after a forward transform, with the type the reference leaves there (:203)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(threshold)


def inverse_threshold_lin(threshold_db):
    """The threshold of the inverse comparison, with the type the reference gives it (:227)."""
    return 10.0 ** (threshold_db / 10.0)


class InverseExpectation:
    def __init__(self, value, threshold, zeros, near):
        self.value = value  # 10^(R/10) in float64
        self.threshold = threshold  # the float64 number a float32 value is compared with
        self.zeros = zeros  # value < threshold, decided on the float64 value
        self.near = near  # |value - threshold| within the bar: a float32 evaluation may decide either way

    def near_share(self):
        return float(np.count_nonzero(self.near)) / max(1, self.near.size)


def db_inverse(R, threshold, zerovalue, bar=0.0):
    """``threshold`` in dB, as the caller passes it.  ``bar``: spacings within which the decision is left open."""
    del zerovalue
    R = np.asarray(R)
    with np.errstate(over="ignore", invalid="ignore"):
        value = 10.0 ** (R.astype(np.float64) / 10.0)
    thr = compared_with(inverse_threshold_lin(threshold), F32)
    with np.errstate(invalid="ignore"):
        zeros = value < thr
        near = np.abs(value - thr) <= bar * np.maximum(spacing32(value), spacing32(thr))
    return InverseExpectation(value, thr, zeros, near & np.isfinite(value))


def deviation(got32, want64, where=None):
    """(worst deviation in float32 spacings of the float64 value, number of elements that had to be equal and are not).

    Where the float64 value is finite and within float32's range the float32 result is measured; where it is NaN, +-inf
    or rounds to +-inf the result must be exactly that."""
    got = np.asarray(got32)
    assert got.dtype == F32, got.dtype
    want = np.asarray(want64, dtype=np.float64)
    sel = np.ones(want.shape, bool) if where is None else np.asarray(where, bool)
    with np.errstate(over="ignore"):
        want32 = want.astype(F32)
    measured = sel & np.isfinite(want32)
    exact = sel & ~measured
    wrong = int(np.count_nonzero(~((got[exact] == want32[exact]) | (np.isnan(got[exact]) & np.isnan(want32[exact])))))
    if not measured.any():
        return 0.0, wrong
    with np.errstate(invalid="ignore"):
        dev = np.abs(got[measured].astype(np.float64) - want[measured]) / spacing32(want[measured])
    dev[~np.isfinite(got[measured])] = np.inf
    return float(dev.max()), wrong


def stats(a):
    """min / max over the finite values (+inf / -inf if there is none), counts of non-finite, -inf and +inf values, and
    np.nanmin (NaN if there is no value that is not NaN)."""
    a = np.asarray(a).ravel()
    fin = a[np.isfinite(a)]
    rest = a[~np.isnan(a)]
    return {
        "min_finite": float(fin.min()) if fin.size else float("inf"),
        "max_finite": float(fin.max()) if fin.size else float("-inf"),
        "nonfinite": int(a.size - fin.size),
        "neg_inf": int(np.count_nonzero(a == -np.inf)),
        "pos_inf": int(np.count_nonzero(a == np.inf)),
        "nanmin": float(rest.min()) if rest.size else float("nan"),
    }


# ---- inputs -------------------------------------------------------------------------------------------------------------


def threshold_forms(value):
    """The same number as a Python float, numpy.float32, numpy.float64 and, where integral, a Python int."""
    forms = [("float", float(value)), ("f32", F32(value)), ("f64", np.float64(value))]
    if float(value) == int(value):
        forms.append(("int", int(value)))
    return forms


def rates(n, seed):
    """Continuous log-uniform rain rates, 0.01 ... 300 mm/h."""
    rng = np.random.default_rng(seed)
    return (10.0 ** rng.uniform(-2.0, np.log10(300.0), n)).astype(F32)


def decibels(n, seed):
    """Continuous uniform dB values, -20 ... 60."""
    return np.random.default_rng(seed).uniform(-20.0, 60.0, n).astype(F32)


def quantised(threshold):
    """Levels 0 ... 199 of a product quantised in steps of float32(threshold), each with its two float32 neighbours:
    level 1 sits exactly on the float32 threshold."""
    levels = np.arange(200, dtype=F32) * F32(threshold)
    assert levels.dtype == F32
    return np.stack([np.nextafter(levels, F32(-np.inf)), levels, np.nextafter(levels, F32(np.inf))], axis=1).ravel()


def rate_specials():
    return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -0.05, FLT_MIN, SUBNORMAL, FLT_MAX, 0.05, 0.1, 1.0, 100.0,
                     np.nan], dtype=F32)


def decibel_specials():
    return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 10.0, 20.0, -20.0, 60.0, 0.5, -10.0, np.nan], dtype=F32)


def decibel_extremes():
    # -400 dB gives a subnormal (1e-40), -379 dB the smallest normals, 385 dB stays below FLT_MAX, 390 dB overflows to +inf
    return np.array([-400.0, -379.0, -379.5, 385.0, 390.0, -440.0, 0.0], dtype=F32)


def stack():
    """The (3, 37, 53) stack of rates whose planes 1 and 2 start off 16-byte alignment."""
    return rates(int(np.prod(STACK_SHAPE)), 53).reshape(STACK_SHAPE)


def forward32(R, threshold, zerovalue):
    """The forward transform as the reference evaluates it, in float32 (input of the round trips)."""
    out = np.array(R, dtype=F32)
    zeros = less_than(out, threshold)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[~zeros] = 10.0 * np.log10(out[~zeros])
    out[zeros] = zerovalue
    return out


class Case:
    """One call of dB_transform: ``R`` float32, ``threshold`` the object the caller passes (dB for the inverse)."""

    def __init__(self, name, inverse, R, threshold, zerovalue, kind):
        self.name, self.inverse, self.R, self.threshold, self.zerovalue, self.kind = name, inverse, R, threshold, zerovalue, kind
        self.R.setflags(write=False)

    @property
    def continuous(self):
        return self.kind == "continuous"

    @property
    def bar_scale(self):
        """1 for dB values within -20 ... 60, the range the bars are measured on.  Beyond it the inverse bar grows with
        the argument: ``R / 10`` is rounded to float32 before the power, which moves 10^(R/10) by up to
        |R / 10| ln(10) / 2 of its spacings - 6.9 of the 7.9 measured at 60 dB - and that term is linear in |R|."""
        if self.kind != "extreme":
            return 1.0
        return max(1.0, float(np.abs(self.R[np.isfinite(self.R)]).max()) / 60.0)

    def metadata(self):
        return {"transform": "dB" if self.inverse else None, "unit": "mm/h"}

    def __repr__(self):
        return "Case(%s)" % self.name


_CASES = None


def cases():
    """The deterministic list of named inputs; built once, arrays read-only."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []

    def add(name, inverse, R, threshold, zerovalue=None, kind="continuous"):
        if zerovalue is None:
            zerovalue = INVERSE_ZERO if inverse else FORWARD_ZERO
        out.append(Case(name, inverse, np.ascontiguousarray(R, dtype=F32), threshold, zerovalue, kind))

    # sizes: body / tail, a looping thread, the grid stride, the planes of the misaligned stack
    for k, n in enumerate(SIZES + (STATS_LOOP, GRID_STRIDE)):
        add("fwd-rates-n%d" % n, False, rates(n, 100 + k), 0.1)
        add("inv-db-n%d" % n, True, decibels(n, 200 + k), -10.0)
    planes = stack()
    for k in range(STACK_SHAPE[0]):
        add("fwd-stack-plane%d" % k, False, planes[k], 0.1)
        add("inv-stack-plane%d" % k, True, forward32(planes[k], 0.1, -15.0), np.float64(-10.0))
    # threshold types on a continuous field
    for form, thr in threshold_forms(0.5) + [("int1", 1)]:
        add("fwd-rates-thr0.5-%s" % form, False, rates(4099, 300), thr)
    for form, thr in threshold_forms(-10.0):
        add("inv-db-thr-10-%s" % form, True, decibels(4099, 301), thr)
    # quantised products: the lowest level sits on the threshold
    for value in THRESHOLDS + (1,):
        for form, thr in threshold_forms(value):
            q = quantised(value)
            add("fwd-quantised-%s-%s" % (value, form), False, q, thr, kind="quantised")
            # the ordinary round trip: the inverse threshold is what the forward call left in the metadata
            zv = forward_threshold_db(thr) - 5
            add("roundtrip-quantised-%s-%s" % (value, form), True, forward32(q, thr, zv), forward_threshold_db(thr),
                kind="roundtrip")
    # special values
    sp = rate_specials()
    for form, thr in threshold_forms(0.1):
        add("fwd-specials-thr0.1-%s" % form, False, sp, thr, kind="special")
    for form, thr in threshold_forms(0.0):
        add("fwd-specials-thr0-%s" % form, False, sp, thr, kind="special")  # log10(0) = -inf is kept
    for form, thr in threshold_forms(-1.0):
        add("fwd-specials-thr-1-%s" % form, False, sp, thr, kind="special")  # log10 of a negative value: NaN
    dsp = decibel_specials()
    for form, thr in threshold_forms(-10.0):
        add("inv-specials-thr-10-%s" % form, True, dsp, thr, kind="special")
    # threshold 0: subnormal results are kept; outside -20 ... 60 dB, so not part of the measured bar (Case.bar_scale)
    add("inv-extremes-thr-500", True, decibel_extremes(), -500.0, kind="extreme")
    add("inv-exact-0-10-20", True, np.array([0.0, 10.0, 20.0], F32), -10.0, kind="special")
    # dB 0 gives exactly 1; 10^(1e-9) is above 1 in float64 and rounds to 1 in float32
    add("inv-isolating-float", True, np.array([0.0, 10.0, 20.0], F32), 1e-8, zerovalue=0.0, kind="isolating")
    add("inv-isolating-f64", True, np.array([0.0, 10.0, 20.0], F32), np.float64(1e-8), zerovalue=0.0, kind="isolating")
    _CASES = out
    return out


ISOLATING_WANT = {"inv-isolating-float": [1.0, 10.0, 100.0], "inv-isolating-f64": [0.0, 10.0, 100.0]}


def expectation(case, bar=0.0):
    if case.inverse:
        return db_inverse(case.R, case.threshold, case.zerovalue, bar)
    return db_forward(case.R, case.threshold, case.zerovalue)


def stats_cases():
    """(name, float32 array) for the reductions: every size, clean / NaN and +inf / -inf in the last element, and the
    degenerate fields."""
    out = []
    for k, n in enumerate(SIZES + (STATS_LOOP, GRID_STRIDE)):
        base = rates(n, 400 + k) - F32(3.0)  # negative values too
        out.append(("clean-n%d" % n, base))
        holes = base.copy()
        holes[n // 3] = np.nan
        holes[n // 2] = np.inf
        out.append(("nan-pinf-n%d" % n, holes))
        low = holes.copy()
        low[-1] = -np.inf
        out.append(("ninf-last-n%d" % n, low))
    out.append(("all-nan", np.full(5, np.nan, F32)))
    out.append(("all-pinf", np.full(5, np.inf, F32)))
    out.append(("nan-and-pinf", np.array([np.nan, np.inf, np.nan], F32)))
    out.append(("empty", np.zeros(0, F32)))
    return out


# ---- conversion patterns ------------------------------------------------------------------------------------------------


def wide_pattern():
    """float64 values whose narrowing exercises round-to-nearest-even, overflow and float32's subnormal range."""
    e = 2.0 ** -24  # half a float32 spacing at 1
    fmax = FLT_MAX
    tiny = 2.0 ** -149  # the smallest float32 subnormal
    vals = [1.0 + e, 1.0 + 3 * e, 1.0 + 5 * e,  # ties: to 1, to 1 + 4e, to 1 + 4e
            1.0 + e + 2.0 ** -50, 1.0 + e - 2.0 ** -50, 1.0 + 3 * e + 2.0 ** -50, 1.0 + 3 * e - 2.0 ** -50,  # just off a tie
            -(1.0 + e), -(1.0 + 3 * e),
            fmax, fmax + 2.0 ** 103 * (1.0 - 2.0 ** -20), fmax + 2.0 ** 103, 1e39, -1e39, 1e300,  # half a spacing past FLT_MAX: +-inf
            -(fmax + 2.0 ** 103),
            1e-40, -1e-40, FLT_MIN * (1.0 - 2.0 ** -25), FLT_MIN * (1.0 - 2.0 ** -24),  # subnormal range
            tiny / 2, 3 * tiny / 2, 5 * tiny / 2, tiny / 2 * (1 + 2.0 ** -40), tiny / 4, 1e-320,  # ties to 0, 2 tiny, 2 tiny
            np.nan, 0.0, -0.0, np.inf, -np.inf, 0.1, 300.0, -15.0, 1.0 / 3.0]
    rng = np.random.default_rng(700)
    return np.concatenate([np.array(vals, np.float64), rng.standard_normal(29) * 10.0 ** rng.uniform(-30, 30, 29)])


def narrow_pattern():
    rng = np.random.default_rng(701)
    vals = [np.nan, 0.0, -0.0, np.inf, -np.inf, FLT_MAX, -FLT_MAX, FLT_MIN, SUBNORMAL, -SUBNORMAL, 2.0 ** -149,
            0.1, 0.7, 1.0 / 3.0]
    return np.concatenate([np.array(vals, np.float32), (rng.standard_normal(50) * 10.0 ** rng.uniform(-20, 20, 50)).astype(np.float32)])


# ---- bars ---------------------------------------------------------------------------------------------------------------


def stored(value):
    """A measured value as the JSON holds it: four significant digits."""
    return float("%.4g" % value)


def measure(ref_db_transform):
    """{direction: (worst deviation of the reference from the float64 restatement in float32 spacings, case name)} over
    ``cases()`` (rates 0.01 ... 300 mm/h and the special values forwards, -20 ... 60 dB backwards), on the elements the
    reference did not set to ``zerovalue``."""
    worst = {"forward": (0.0, None), "inverse": (0.0, None)}
    for c in cases():
        if c.kind == "extreme":
            continue
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got, _ = ref_db_transform(c.R.copy(), c.metadata(), threshold=c.threshold, zerovalue=c.zerovalue, inverse=c.inverse)
        exp = expectation(c)
        # no case's zerovalue is a value the transform can produce from its input
        kept = ~(got == F32(c.zerovalue)) if c.inverse else ~exp.zeros
        dev, _ = deviation(got, exp.value, kept)
        key = "inverse" if c.inverse else "forward"
        if dev > worst[key][0]:
            worst[key] = (dev, c.name)
    return worst


_BARS = None


def load_bars():
    global _BARS
    if _BARS is None:
        with open(BARS_JSON) as fh:
            _BARS = json.load(fh)
    return _BARS


def bar(direction, bars=None):
    """The device's bar in float32 spacings of the float64 value: BAR_FACTOR x the reference's own deviation."""
    return float((bars or load_bars())[direction]["bar"])


def write_bars(ref_db_transform, path=BARS_JSON):
    doc = {"unit": "spacing of the float32 nearest to the float64 value",
           "measured_with": "pysteps.utils.transformation.dB_transform (float32) against helpers/elementwise.py::db_forward / "
                            "db_inverse (float64), on the CPU, over helpers/elementwise.py::cases",
           "bar_factor": BAR_FACTOR}
    for direction, (dev, where) in measure(ref_db_transform).items():
        dev = stored(dev)
        doc[direction] = {"measured": dev, "bar": BAR_FACTOR * dev, "worst_case": where}
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return doc


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from oracle import build_ref

    build_ref.activate()
    from pysteps.utils.transformation import dB_transform

    print(json.dumps(write_bars(dB_transform), indent=1, sort_keys=True))
