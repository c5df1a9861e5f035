"""Hard planes and a wide oracle for the (mean, population std) reduction of whole float64 planes (``psh::moments``,
csrc/noise_adj.hip: level statistics and field mean of the cascade decomposition, the noise filter's standardisation,
``np.std(N)`` of the noise adjustment's prepare stage).

The planes are the ones a one-pass ``E[v^2] - E[v]^2`` with a shift taken from the data goes wrong on: with
``d = |x[0] - mean| / std`` such a sum loses about ``d^2`` of the significand, and ``d`` reaches sqrt(pixels) where one
intense value sits on the plane's first pixel.  Every family is built at the smallest shapes of the suite (a power of
two, both sides odd, even sides that are no powers of two) and, as 1-D planes, at the sizes around the reduction's
launch: one lane, one wave (64), one block (256) and one full grid stride (512 blocks x 256 threads = 131072).

The oracle is a two-pass mean and population std in ``numpy.longdouble`` (64-bit significand), rounded to float64 once
at the end; where longdouble is no wider than that (``nmant < 63``) the planes of at most 4096 elements are evaluated
in exact rationals instead and the larger ones raise :class:`OracleUnavailable`.

The bars follow tests/test_noise_adj_gpu.py: 5 x what the reference's own float64 ``np.mean`` / ``np.std`` deviate from
the oracle, relative to the plane's std, per case and per statistic, with a floor of 16 x 2^-53 (the final roundings
of the mean, the variance and the square root, where NumPy happens to hit the oracle exactly).  No std bar may exceed
the project's recorded ``5 x deviation_moments`` (tests/golden/noise_adj_reference.npz): tests/test_moments_cpu.py
asserts that, it is a condition on the planes and not a measurement of any device.
"""

import functools
import math
import os
from fractions import Fraction

import numpy as np

SHAPES = ((64, 64), (67, 129), (128, 96))
GRID_STRIDE = 512 * 256  # elements one sweep of the reduction's grid takes
EDGE_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, GRID_STRIDE - 1, GRID_STRIDE, GRID_STRIDE + 1)
SPIKE = 60.0
SPIKE_ROLLS = ("spike_first", "spike_at_1", "spike_at_63", "spike_at_64", "spike_last", "spike_middle")
HARD_FAMILIES = ("spike_first", "offset_first_outlier", "corner_cell_band", "negative_spike")  # d >= 50 at SHAPES
FAMILIES = ("benign",) + SPIKE_ROLLS + HARD_FAMILIES[1:]
CONSTANTS = (0.0, -15.0, 0.1, 1e4 + 1.0 / 3.0)
NONFINITE = ("nan_first", "nan_last", "posinf_first", "posinf_last", "neginf_first", "neginf_last")
FRACTION_MAX = 4096  # elements the exact-rational route takes
U = 2.0 ** -53
FLOOR = 16.0 * U
BAND_CENTRE, BAND_WIDTH = 0.35, 0.12  # cycles / pixel, Gaussian band of corner_cell_band


class OracleUnavailable(Exception):
    """numpy.longdouble is too narrow here and the plane is too large for exact rationals."""


def wide_longdouble():
    return np.finfo(np.longdouble).nmant >= 63


def _seed(name, size):
    return [sum(ord(c) * (i + 1) for i, c in enumerate(name)), int(size)]


def _roll_of(name, size):
    return {"spike_first": 0, "spike_at_1": 1, "spike_at_63": 63, "spike_at_64": 64, "spike_last": size - 1,
            "spike_middle": size // 2}[name]


def band_pass(field, centre=BAND_CENTRE, width=BAND_WIDTH):
    """A Gaussian band-pass around ``centre`` cycles per pixel applied to a 2-D field (NumPy transforms)."""
    m, n = field.shape
    k = np.hypot(np.fft.fftfreq(m)[:, None], np.fft.rfftfreq(n)[None, :])
    return np.fft.irfft2(np.fft.rfft2(field) * np.exp(-0.5 * ((k - centre) / width) ** 2), s=(m, n))


@functools.lru_cache(maxsize=None)
def plane(family, shape):
    """The plane of a family at a shape (a tuple; 1-D planes: ``(size,)``), float64, read-only."""
    size = int(np.prod(shape))
    if family in SPIKE_ROLLS:  # one plane, rolled
        x = 0.01 * np.random.default_rng(_seed("spike", size)).standard_normal(size)
        x[0] = SPIKE
        x = np.roll(x, _roll_of(family, size)).reshape(shape)
    else:
        rng = np.random.default_rng(_seed(family, size))
        if family == "benign":
            x = 3.0 * rng.standard_normal(shape)
        elif family == "negative_spike":
            x = 0.01 * rng.standard_normal(shape)
            x.flat[0] = -SPIKE
        elif family == "offset_first_outlier":
            x = 0.01 * rng.standard_normal(shape) + 1e4
            x.flat[0] = 1e4 + 5.0
        elif family == "corner_cell_band":
            cell = np.full(shape, -15.0)
            cell[0, 0] = 50.0
            x = band_pass(cell)
        else:
            raise ValueError(family)
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.setflags(write=False)
    return x


def constant_plane(c, shape):
    return np.full(shape, c, dtype=np.float64)


def nonfinite_plane(kind, shape):
    """The benign plane of the shape with one NaN / +Inf / -Inf as its first or its last element."""
    what, where = kind.split("_")
    x = plane("benign", shape).copy()
    x.flat[0 if where == "first" else x.size - 1] = {"nan": np.nan, "posinf": np.inf, "neginf": -np.inf}[what]
    return x


def shape_cases():
    """(family, shape) of every family at the three 2-D shapes."""
    return [(f, s) for s in SHAPES for f in FAMILIES]


def edge_cases():
    """(family, (size,)) of the 1-D planes around the launch's edges."""
    return [(f, (n,)) for n in EDGE_SIZES for f in ("spike_first", "benign")]


def case_id(family, shape):
    return "%s_%s" % (family, "x".join(str(s) for s in shape))


# ---- the oracle ---------------------------------------------------------------------------------------------------

def _oracle_longdouble(x):
    w = np.asarray(x, dtype=np.longdouble).reshape(-1)
    n = np.longdouble(w.size)
    first = np.sum(w) / n
    r = w - first  # second pass: what the first mean missed, and the squares about it
    corr = np.sum(r) / n
    var = np.sum(r * r) / n - corr * corr
    return float(first + corr), float(np.sqrt(max(var, np.longdouble(0.0))))


def _sqrt_fraction(v, bits=160):
    """sqrt of a non-negative Fraction to ``bits`` bits (floor), as a Fraction."""
    if v == 0:
        return Fraction(0)
    shift = max(0, bits - (v.numerator.bit_length() - v.denominator.bit_length()) // 2)
    return Fraction(math.isqrt((v.numerator << (2 * shift)) // v.denominator), 1 << shift)


def oracle_fraction(x):
    """(mean, population std) in exact rationals, each rounded to float64 once (the std: the square root taken to 160
    bits first)."""
    vals = [Fraction(float(v)) for v in np.asarray(x, dtype=np.float64).reshape(-1)]
    if len(vals) > FRACTION_MAX:
        raise OracleUnavailable("exact rationals take planes of at most %d elements, not %d" % (FRACTION_MAX, len(vals)))
    n = len(vals)
    mean = sum(vals, Fraction(0)) / n
    var = sum(((v - mean) ** 2 for v in vals), Fraction(0)) / n
    return float(mean), float(_sqrt_fraction(var))


def oracle(x):
    """(mean, population std) of a finite plane as float64, from arithmetic wide enough that the pair is the correctly
    rounded one up to a double rounding."""
    x = np.asarray(x, dtype=np.float64)
    if wide_longdouble():
        return _oracle_longdouble(x)
    if x.size <= FRACTION_MAX:
        return oracle_fraction(x)
    raise OracleUnavailable("numpy.longdouble has a %d-bit significand here (64 needed) and the plane of %d elements is "
                            "beyond the %d that exact rationals take" % (np.finfo(np.longdouble).nmant + 1, x.size, FRACTION_MAX))


@functools.lru_cache(maxsize=None)
def case_oracle(family, shape):
    return oracle(plane(family, shape))


# ---- bars -----------------------------------------------------------------------------------------------------------

def scale_of(mean, std):
    """What the errors of a plane are relative to: its std; a plane without spread (one element): |mean|."""
    return std if std > 0.0 else (abs(mean) if mean != 0.0 else 1.0)


def bars(x, want=None):
    """(bar of the mean, bar of the std) of a plane: 5 x the deviation of np.mean / np.std from the oracle relative to
    the plane's std, not below FLOOR.  Also returns the two deviations themselves."""
    x = np.asarray(x, dtype=np.float64)
    mean, std = oracle(x) if want is None else want
    scale = scale_of(mean, std)
    dev = (abs(float(np.mean(x)) - mean) / scale, abs(float(np.std(x)) - std) / scale)
    return (max(5.0 * dev[0], FLOOR), max(5.0 * dev[1], FLOOR)), dev


def errors(got, want):
    """(error of the mean, error of the std) of a device pair against the oracle's, relative to the plane's std."""
    scale = scale_of(*want)
    return abs(float(got[0]) - want[0]) / scale, abs(float(got[1]) - want[1]) / scale


def first_pixel_distance(x):
    """d = |x[0] - mean| / std."""
    x = np.asarray(x, dtype=np.float64)
    mean, std = oracle(x)
    return abs(float(x.flat[0]) - mean) / std


def cap():
    """The project's bar for this kind of quantity: 5 x deviation_moments of tests/golden/noise_adj_reference.npz."""
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "noise_adj_reference.npz")
    return 5.0 * float(np.load(golden, allow_pickle=False)["deviation_moments"])


def ulps(got, want):
    """|got - want| in units in the last place of ``want``."""
    return abs(float(got) - float(want)) / float(np.spacing(abs(float(want)))) if want != 0.0 else (0.0 if got == 0.0 else np.inf)


# ---- fields for the callers ----------------------------------------------------------------------------------------

def cell_field(shape, centred):
    """-15 dB with one intense cell (Gaussian, 1.5 pixels wide, 50 dB at its peak) on pixel (0, 0), or the same field
    rolled to the centre."""
    m, n = shape
    dy = np.minimum(np.arange(m), m - np.arange(m))[:, None]
    dx = np.minimum(np.arange(n), n - np.arange(n))[None, :]
    field = -15.0 + 65.0 * np.exp(-0.5 * (dy * dy + dx * dx) / 1.5 ** 2)
    return np.roll(field, (m // 2, n // 2), axis=(0, 1)) if centred else field


def radial_filter(shape, width=0.25):
    """A smooth radial low-pass filter on the rfft2 half spectrum, (m, n // 2 + 1)."""
    m, n = shape
    k = np.hypot(np.fft.fftfreq(m)[:, None], np.fft.rfftfreq(n)[None, :])
    return np.exp(-(k / width) ** 2)


def delta_noise(shape, seed=5):
    """White noise 1e-3 N(0, 1) plus a delta of 1.0 at (0, 0): filtered with :func:`radial_filter`, the output's first
    pixel is its peak."""
    x = 1e-3 * np.random.default_rng(seed).standard_normal(shape)
    x[0, 0] += 1.0
    return x
