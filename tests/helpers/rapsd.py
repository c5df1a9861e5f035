"""Host restatement of the radially averaged power spectrum (pysteps/utils/spectral.py:100-180), independent of the
product: the bins come from the radius grid built as the reference builds it (``round(sqrt(xc**2 + yc**2))`` in
floating point; the plane is sorted by it once, which selects what the reference's mask ``r_grid == r`` selects without
a pass over the plane per radius), every bin's terms are added with ``math.fsum``
(exact, one rounding) and divided in rational arithmetic (one more rounding).  Two evaluators, both returning
``(means float64 (nb,), counts int64 (nb,))``:

``exact_full(psd)``      of a shifted power plane (float32, float64 or longdouble, taken as the numbers they are);
``exact_half(X, m, n)``  of a complex128 half spectrum ``(m, n//2+1)``: ``|X|**2 / (m n)`` with re**2 and im**2 split
                         into a rounded product and its exact error (Dekker), the mirrored columns counted twice.

Also the integer bin rule the device uses, restated (``bin_rule``), and the test fields.
"""
import math
from fractions import Fraction

import numpy as np

# golden cases: name -> (shape, seed)
CASES = {"p8x8": ((8, 8), 11), "p9x9": ((9, 9), 12), "p8x9": ((8, 9), 13), "p9x8": ((9, 8), 14), "p2x64": ((2, 64), 15),
         "p129x140": ((129, 140), 16), "p257x311": ((257, 311), 17), "p640x710": ((640, 710), 18), "p512x512": ((512, 512), 19)}
# shapes the device tests add: the two that strain the bin count, and one that is prime-ish on both sides
EXTRA_SHAPES = [(8192, 128), (128, 8192), (1226, 761)]


def bins(m, n):
    l = max(m, n)
    return l // 2 + 1 if l % 2 == 1 else l // 2


def centred(s):
    """The centred integer coordinates of a side (pysteps/utils/arrays.py compute_centred_coord_array)."""
    return np.arange(-int(s / 2), int(s / 2)) if s % 2 == 0 else np.arange(-int(s / 2), int(s / 2) + 1)


def r_grid_full(m, n):
    yc, xc = centred(m)[:, None], centred(n)[None, :]
    return np.sqrt(xc * xc + yc * yc).round()


def r_grid_half(m, n):
    ky = np.array([i if i <= (m - 1) // 2 else i - m for i in range(m)])[:, None]
    kx = np.arange(n // 2 + 1)[None, :]
    return np.sqrt(kx * kx + ky * ky).round()


def half_weights(n):
    w = np.full(n // 2 + 1, 2, dtype=np.int64)
    w[0] = 1
    if n % 2 == 0:
        w[n // 2] = 1
    return w


def bin_rule(N):
    """The bin of N = kx**2 + ky**2 in integer arithmetic: the r with r**2 - r < N <= r**2 + r (0 for N = 0)."""
    N = np.asarray(N, dtype=np.int64)
    r = np.floor(np.sqrt(N.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > N, r - 1, r)
    r = np.where((r + 1) * (r + 1) <= N, r + 1, r)
    return np.where(N > r * r + r, r + 1, r)


def _doubles(values):
    """The values as float64 numbers whose exact sum is theirs (a longdouble is split into two)."""
    values = np.asarray(values)
    if values.dtype == np.longdouble and np.finfo(np.longdouble).nmant > 52:
        hi = values.astype(np.float64)
        return np.concatenate([hi, (values - hi.astype(np.longdouble)).astype(np.float64)])
    return values.astype(np.float64)


def _mean(terms, divisor):
    return float(Fraction(math.fsum(terms)) / divisor)


def exact_full(psd):
    psd = np.asarray(psd)
    m, n = psd.shape
    r_grid = r_grid_full(m, n)
    nb = bins(m, n)
    means, counts = np.empty(nb, dtype=np.float64), np.empty(nb, dtype=np.int64)
    order = np.argsort(r_grid, axis=None, kind="stable")
    sorted_r = r_grid.ravel()[order]
    flat = psd.ravel()[order]
    edges = np.searchsorted(sorted_r, np.arange(nb + 1))
    for r in range(nb):
        vals = flat[edges[r]:edges[r + 1]]
        counts[r] = vals.size
        means[r] = _mean(_doubles(vals), int(vals.size))
    return means, counts


def _square_parts(a):
    """a * a = p + e exactly (Dekker's product; no overflow at these magnitudes)."""
    p = a * a
    c = 134217729.0 * a
    hi = c - (c - a)
    lo = a - hi
    return p, ((hi * hi - p) + 2.0 * hi * lo) + lo * lo


def exact_half(X, m, n):
    X = np.asarray(X, dtype=np.complex128)
    assert X.shape == (m, n // 2 + 1)
    r_grid = r_grid_half(m, n)
    weights = np.broadcast_to(half_weights(n)[None, :], X.shape)
    nb = bins(m, n)
    parts = np.stack(_square_parts(X.real.copy()) + _square_parts(X.imag.copy()), axis=-1) * weights[..., None]  # x 1 or 2: exact
    means, counts = np.empty(nb, dtype=np.float64), np.empty(nb, dtype=np.int64)
    order = np.argsort(r_grid, axis=None, kind="stable")
    sorted_r = r_grid.ravel()[order]
    parts, w = parts.reshape(-1, 4)[order], weights.ravel()[order]
    edges = np.searchsorted(sorted_r, np.arange(nb + 1))
    for r in range(nb):
        counts[r] = int(w[edges[r]:edges[r + 1]].sum())
        means[r] = _mean(parts[edges[r]:edges[r + 1]].ravel(), int(counts[r]) * m * n)
    return means, counts


def relative(got, want):
    """Largest per-bin relative difference; a bin whose expected mean is 0 must be 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    zero = want == 0
    assert np.array_equal(got[zero], want[zero])
    return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]))) if (~zero).any() else 0.0


def rain_field(m, n, seed):
    """A rain-like field: 40 % wet pixels with gamma-distributed rates, multiples of 1/8 (every value is a float32
    number, so a float64 run sees the same numbers widened)."""
    rs = np.random.RandomState(seed)
    rate = rs.gamma(0.5, 4.0, size=(m, n))
    wet = rs.random_sample((m, n)) < 0.4
    return np.where(wet, np.round(rate * 8.0) / 8.0, 0.0).astype(np.float32)


def power_law_field(m, n, seed, slope=-1.5):
    """Gaussian noise whose amplitude spectrum falls as k**slope, standardized: a spectrum a parametric noise filter
    can be fitted to (a rain_field is white)."""
    rs = np.random.RandomState(seed)
    ky, kx = np.fft.fftfreq(m)[:, None] * m, np.fft.rfftfreq(n)[None, :] * n
    k = np.sqrt(kx * kx + ky * ky)
    k[0, 0] = 1.0
    field = np.fft.irfft2(np.fft.rfft2(rs.randn(m, n)) * k ** slope, s=(m, n))
    return (field - field.mean()) / field.std()


def cosine_field(m, n, a, b):
    """cos(2 pi (a x / n + b y / m)): all power at (ky, kx) = +-(b, a), bin ``bin_rule(a*a + b*b)``."""
    y, x = np.arange(m)[:, None], np.arange(n)[None, :]
    return np.cos(2.0 * np.pi * (a * x / n + b * y / m))


def constant_field(m, n, value=3.0):
    return np.full((m, n), value, dtype=np.float64)


def shifted_power(field):
    """The reference's expression for the shifted power plane, through numpy.fft."""
    psd = np.fft.fftshift(np.fft.fft2(field))
    return np.abs(psd) ** 2 / psd.size
