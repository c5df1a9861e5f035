"""The cases of tests/test_fft_pointwise_*.py: shapes named with the path of csrc/fft.hip they pin, and the input
families every shape is run with.  A heavy side is always paired with a tiny one."""

import functools

import numpy as np

from helpers import fft_pointwise as fp

# (shape, what it pins)
SHAPES = [
    # fft_lds structure: logn 1 .. 8 on both axes - the first radix-2 layer of an odd logn, 0 / 1 / 2 fft_pass16 rounds,
    # the final pair of layers
    ((2, 2), "fft_lds logn 1 x 1: the radix-2 layer alone; one column group, fewer than XCDs"),
    ((4, 8), "fft_lds logn 2 (final pair alone) x logn 3 (radix-2 + final pair)"),
    ((16, 2), "fft_lds logn 4: one fft_pass16 round alone"),
    ((8, 32), "fft_lds logn 3 x logn 5 (radix-2 + one fft_pass16)"),
    ((64, 128), "fft_lds logn 6 (fft_pass16 + final pair) x logn 7 (radix-2 + fft_pass16 + final pair)"),
    ((256, 16), "fft_lds logn 8: two fft_pass16 rounds"),
    # fft_cols_c2c, one sweep
    ((512, 6), "fft_cols_c2c cols = 2 at 512 points; chirp rows"),
    ((4096, 6), "fft_cols_c2c cols = 2 at 4096 points (the LDS limit of two columns)"),
    ((1024, 6), "fft_cols_c2c narrow form (one column, 256 threads) at 1024 points"),
    ((2048, 6), "fft_cols_c2c narrow form at 2048 points"),
    ((512, 4), "rfft2 nc = 3: the last group of two columns has one live column (c < live)"),
    ((128, 12), "rfft2 nc = 7: odd nc, four groups"),
    ((512, 2), "nc = 2: one group, fewer groups than XCDs (g >= groups)"),
    ((128, 34), "rfft2 nc = 18: nine groups, not a multiple of the XCD count; c2c 17 groups"),
    ((1024, 34), "narrow form with 18 / 34 groups, not a multiple of the XCD count"),
    # row pairs: the last row alone in its pair
    ((3, 8), "odd m: rb = min(ra + 1, m - 1), two workgroups"),
    ((127, 16), "odd m, chirp columns"),
    ((4095, 2), "odd m at the chirp limit"),
    # rows at the LDS limit
    ((2, 8192), "8192-point rows: 128 KiB of LDS, 1024 threads"),
    ((3, 8192), "8192-point rows with an odd m and chirp columns"),
    # fft_cols_step, the default path at 8192 rows
    ((8192, 2), "fft_cols_step: nc = 2 / n = 2, one partial column tile"),
    ((8192, 6), "fft_cols_step with chirp rows: nc = 4, fewer than one column tile"),
    ((8192, 34), "fft_cols_step: nc = 18, two tiles, the second partial; c2c three tiles"),
    # chirp-z
    ((3, 5), "chirp-z both axes, M = 8 / 16"),
    ((7, 2), "chirp-z columns, plain rows of two points"),
    ((2, 7), "chirp-z rows, odd n: no Nyquist bin"),
    ((17, 31), "chirp-z primes, M = 64"),
    ((1023, 2), "chirp-z below a power of two: M = 2048"),
    ((1025, 2), "chirp-z above a power of two: M jumps to 4096"),
    ((2047, 3), "chirp-z below a power of two: M = 4096"),
    ((2049, 3), "chirp-z above a power of two: M jumps to 8192"),
    ((4095, 6), "chirp-z at its limit, M = 8192, columns"),
    ((6, 4095), "chirp-z at its limit, rows"),
    ((100, 64), "chirp columns, plain rows"),
    ((64, 100), "plain columns, chirp rows"),
    ((640, 710), "the radar composite"),
]
# column lengths the four-step kernels take only with PYSTEPS_HIP_FFT_FOURSTEP=2 (helpers/fft_fourstep_child.py):
# log1 / log2 = 5 / 5, 5 / 6, 6 / 6 and per_col 4 / 4, 4 / 2, 2 / 2 against 6 / 7 and 2 / 1 at 8192
FOURSTEP_SHAPES = [(1024, 2), (1024, 34), (2048, 2), (2048, 34), (4096, 2), (4096, 34)]
# fft_irfft2_weighted with weights != nullptr: both column kernels, plain and chirp
WEIGHTED_SHAPES = [(64, 128), (100, 64), (1024, 6), (8192, 6), (8192, 34)]


def shape_name(shape):
    return "%dx%d" % tuple(shape)


def _seed(shape):
    return int(shape[0]) * 10007 + int(shape[1])


def _dedupe(points):
    out = []
    for p in points:
        if p not in out:
            out.append(p)
    return out


def impulse_points(shape):
    m, n = shape
    return _dedupe([(0, 0), (m - 1, n - 1), (m // 2, n // 3)])


def tone_bins(shape):
    m, n = shape
    return _dedupe([(0, 0), (1 % m, 1 % n), (m // 2, n // 2), (m - 1, n - 1)])


@functools.lru_cache(maxsize=4)
def fields(shape):
    """name -> (real float64 field, complex128 field), each dense in every row (or an impulse: dense in every bin).
    The family is the name up to the first '@'."""
    from tools import synth

    m, n = shape
    rng = np.random.default_rng(_seed(shape))
    out = {}
    out["noise"] = (rng.standard_normal(shape), rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    out["mean1e6"] = (rng.standard_normal(shape) + 1e6, rng.standard_normal(shape) + 1j * rng.standard_normal(shape) + (1e6 + 1e6j))
    for at in impulse_points(shape):
        x = np.zeros(shape)
        x[at] = 1.0
        out["impulse@%d,%d" % at] = (x, x.astype(np.complex128))
    for at in tone_bins(shape):
        z = fp.tone(shape, at)
        out["tone@%d,%d" % at] = (z.real.astype(np.float64), z.astype(np.complex128))
    rain = synth.rain_field_db(m, n, seed=_seed(shape)).astype(np.float64)
    rain2 = synth.rain_field_db(m, n, seed=_seed(shape) + 1).astype(np.float64)
    out["rain"] = (rain, rain + 1j * rain2)
    for a, b in out.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return out


def family(name):
    return name.split("@")[0]


@functools.lru_cache(maxsize=8)
def inputs(shape, op):
    """name -> the float64 / complex128 input of ``op``.  The spectra of the inverse transforms are the oracle's forward
    results of the same fields, rounded once, plus one set of random spectra that are not Hermitian."""
    m, n = shape
    f = fields(shape)
    if op == "rfft2":
        out = {k: v[0] for k, v in f.items()}
    elif op == "fft2":
        out = {k: v[1] for k, v in f.items()}
    elif op == "irfft2":
        out = {k: v.astype(np.complex128) for k, v in wants(shape, "rfft2").items()}
        rng = np.random.default_rng(_seed(shape) + 7)
        out["nonhermitian"] = rng.standard_normal((m, n // 2 + 1)) + 1j * rng.standard_normal((m, n // 2 + 1))
    elif op == "ifft2":
        out = {k: v.astype(np.complex128) for k, v in wants(shape, "fft2").items()}
        rng = np.random.default_rng(_seed(shape) + 8)
        out["nonhermitian"] = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    else:
        raise ValueError(op)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=8)
def wants(shape, op):
    """name -> the oracle's output, computed once per shape and operation and shared."""
    out = {k: fp.oracle(op, x, shape) for k, x in inputs(shape, op).items()}
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- the weighted inverse ---------------------------------------------------------------------------------------------
N_LEVELS = 3


def weight_banks(shape):
    """name -> (3, m, n // 2 + 1) float64: a Gaussian band-pass bank, all ones, one non-zero row and column per level."""
    m, n = shape
    nc = n // 2 + 1
    ky = np.fft.fftfreq(m)[:, None] * m
    kx = np.fft.rfftfreq(n)[None, :] * n
    r = np.hypot(ky, kx)
    centres = np.geomspace(1.0, max(max(m, n) / 2.5, 2.0), N_LEVELS)
    gauss = np.stack([np.exp(-0.5 * ((np.log(np.maximum(r, 0.5)) - np.log(c)) / 0.45) ** 2) for c in centres])
    gauss[0][r < centres[0]] = 1.0
    cross = np.zeros((N_LEVELS, m, nc))
    for k, (r0, c0) in enumerate([(0, 0), (m // 3, nc - 1), (m - 1, nc // 2)]):
        cross[k, r0, :] = 1.0 + 0.25 * np.cos(np.arange(nc))
        cross[k, :, c0] = 1.0 + 0.25 * np.sin(np.arange(m))
    return {"gauss": gauss, "ones": np.ones((N_LEVELS, m, nc)), "cross": cross}


@functools.lru_cache(maxsize=2)
def weighted_field(shape):
    """Gaussian noise: every bin of its spectrum has the size of the whole array's root mean square, so the rounding of
    the forward transform (which scales with that) stays in proportion to whatever the weights keep."""
    x = np.random.default_rng(_seed(shape) + 21).standard_normal(shape)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=2)
def weighted_wants(shape):
    """(bank, level) -> oracle level, long double"""
    x = weighted_field(shape)
    return {(name, k): fp.oracle("weighted", x, shape, bank[k]) for name, bank in weight_banks(shape).items()
            for k in range(N_LEVELS)}


# ---- yardsticks -------------------------------------------------------------------------------------------------------
def measure(shape, op):
    """family -> {"numpy": (worst err / u, case name), "restated": ...} of one shape and operation over its inputs
    ("restated" only where a side is not a power of two; the families of the weighted inverse are its banks)."""
    chirp = fp.shape_class(shape) == "chirp"
    out = {}

    def take(fam, kind, val, name):
        slot = out.setdefault(fam, {})
        if kind not in slot or val > slot[kind][0]:
            slot[kind] = (val, name)

    if op == "weighted":
        x = weighted_field(shape)
        banks = weight_banks(shape)
        for (bank, k), want in weighted_wants(shape).items():
            name = "%s-%s[%d]" % (shape_name(shape), bank, k)
            take(bank, "numpy", fp.compare(fp.numpy_f64(op, x, shape, banks[bank][k]), want)[0], name)
            if chirp:
                take(bank, "restated", fp.compare(fp.restated(op, x, shape, banks[bank][k]), want)[0], name)
        return out
    want = wants(shape, op)
    for key, x in inputs(shape, op).items():
        name = "%s-%s" % (shape_name(shape), key)
        take(family(key), "numpy", fp.compare(fp.numpy_f64(op, x, shape), want[key])[0], name)
        if chirp:
            take(family(key), "restated", fp.compare(fp.restated(op, x, shape), want[key])[0], name)
    return out


def shapes_of(op):
    """The shapes an operation's yardstick is measured over: the case list and the four-step shapes of the child; the
    weighted inverse on its own shapes and the child's."""
    if op == "weighted":
        return WEIGHTED_SHAPES + FOURSTEP_SHAPES
    return [s for s, _ in SHAPES] + FOURSTEP_SHAPES


def all_measurements():
    """[(shape, op)] in the order that shares the cached oracles: shape by shape"""
    seen, out = set(), []
    for op in fp.OPS:
        for shape in shapes_of(op):
            if (shape, op) not in seen:
                seen.add((shape, op))
                out.append((shape, op))
    order = {s: i for i, s in enumerate(dict.fromkeys(s for s, _ in out))}
    return sorted(out, key=lambda so: (order[so[0]], fp.OPS.index(so[1])))


def bars_from(measured):
    """The content of tests/golden/fft_pointwise_bars.json from {(shape, op): measure(shape, op)}.  Per class and
    operation: C = the largest yardstick value over the class's cases, bar = 4 C.  The same per input family
    ("families"): a spike in the output (the DC bin of a field with a mean, the bin of a tone, the pixel of an impulse) is
    |spike| / rms ~ sqrt(m n) units large, and so is its rounding in any float64 transform - the class's C is set by these
    families, and the dense families are held to their own, far smaller, C as well."""
    classes = {"plain": {}, "chirp": {}}
    for op in fp.OPS:
        worst = {"plain": {}, "chirp": {}}
        for shape in shapes_of(op):
            cls = fp.shape_class(shape)
            for fam, kinds in measured[(shape, op)].items():
                for kind, (val, name) in kinds.items():
                    if fam not in worst[cls] or val > worst[cls][fam][0]:
                        worst[cls][fam] = (val, name, kind)
        for cls, fams in worst.items():
            top = max(fams.values(), key=lambda t: t[0])

            def entry(t):
                c = round(t[0], 3)
                return {"C": c, "bar": round(fp.BAR_FACTOR * c, 3), "worst_case": t[1], "worst_yardstick": t[2]}

            classes[cls][op] = dict(entry(top), families={fam: entry(t) for fam, t in sorted(fams.items())})
    return {
        "bar_factor": fp.BAR_FACTOR,
        "measured_with": "helpers/fft_pointwise_cases.py::bars_from on the CPU: numpy.fft in float64 and, for sides that are "
                         "not powers of two, helpers/fft_pointwise.py::restated (the kernel's chirp-z algorithm in float64), "
                         "each against numpy.fft in long double, over every input of every shape of the case list",
        "unit": "u = 2^-53 * sqrt(mean |oracle output|^2) over the whole output",
        "classes": classes,
    }
