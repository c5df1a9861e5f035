"""Cases, inputs and restatements of pysteps/timeseries/correlation.py ``temporal_autocorrelation`` (test yardstick).

Inputs.  A cascade ``(L, T, m, n)`` is built from a counter-based integer generator (splitmix64 in uint64 arithmetic:
the same bits on every machine) on a binary grid: float64 values are multiples of 2^-45 below 128 in magnitude (52
significant bits, so a product needs 104 and the kernels' error-free products are exercised), float32 values multiples
of 2^-18 below 32.  Sums, differences of two planes (``d = 1``, in either precision) and ``x * 2^45`` are therefore
exact, and the sums a coefficient is made of can be taken in Python integers.  Every level has a mean that is not
small beside its spread (1.5 + 2.5 l), which is what makes ``S_aa - S_a^2 / N`` cancel.

Restatements.  :func:`reference_float64` is the reference's arithmetic (``np.corrcoef`` of the boolean-indexed
planes; ``spectral.corrcoef``; ``_moving_window_corrcoef`` with SciPy's filter) and is held to the goldens by
tests/test_autocorr_cpu.py.  :func:`exact_gamma` takes the sums as integers / rationals and finishes in
``numpy.longdouble``: the number the reference's float64 stands for.
"""

import warnings
from fractions import Fraction

import numpy as np

SHAPES = [(5, 7), (61, 67), (257, 263)]  # less than a wave; odd count: every second float64 plane 8 bytes off; several blocks
LEVELS = [1, 3, 8]
FRAMES = [2, 3, 4]
DTYPES = ["float32", "float64"]
MASKS = ["none", "all", "sparse", "two", "one", "empty"]
VARIANTS = ["plain", "constant", "identical"]
SPECTRAL_SHAPES = [(16, 16), (15, 17), (61, 67)]
WINDOW_SHAPE = (61, 67)
WINDOW_SIGMAS = [1.5, 4]
STORED_SHAPES = [(5, 7), (61, 67)]  # the golden file holds these level-0 float64 series as generated
_GRID = {"float64": 45, "float32": 18}
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix(counter):
    z = counter.astype(np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _grid_noise(count, stream, bits, grid):
    """``count`` values on the grid 2^-grid, uniform in [-2^(bits-1-grid), 2^(bits-1-grid)), as float64."""
    with np.errstate(over="ignore"):
        raw = _splitmix(np.arange(count, dtype=np.uint64) + np.uint64(stream) * np.uint64(0x1000003D1))
    top = (raw >> np.uint64(64 - bits)).astype(np.int64) - (1 << (bits - 1))
    return top.astype(np.float64) * 2.0 ** -grid


def cascade(shape, L, T, dtype, variant="plain"):
    """The case's cascade ``(L, T, m, n)``: per level a common field plus a quarter of a fresh one per frame and of the
    frame before (lag-1 and lag-2 correlations that differ), and the level's offset."""
    grid = _GRID[dtype]
    bits = grid + 1  # |common|, |fresh| < 4 on the grid 2^-(grid - 2)
    npix = shape[0] * shape[1]
    out = np.empty((L, T, npix), dtype=np.float64)
    for l in range(L):
        common = _grid_noise(npix, 1000 * l + 7, bits, grid - 2)
        fresh = [_grid_noise(npix, 1000 * l + 11 + t, bits, grid - 2) for t in range(T + 1)]
        for t in range(T):
            out[l, t] = common + fresh[t + 1] / 4.0 + fresh[t] / 4.0 + (1.5 + 2.5 * l)
    if variant == "constant":
        out[:, -1] = 2.5
    elif variant == "identical":
        out[:, -2] = out[:, -1]
    assert np.array_equal(out, out.astype(dtype).astype(np.float64))  # on the grid: nothing was rounded
    return out.astype(dtype).reshape((L, T) + tuple(shape))


def mask_of(kind, shape):
    """None or a boolean mask: every pixel, about 5 % of them, exactly two, exactly one, none."""
    npix = shape[0] * shape[1]
    if kind == "none":
        return None
    flat = np.zeros(npix, dtype=bool)
    if kind == "all":
        flat[:] = True
    elif kind == "sparse":
        flat = _grid_noise(npix, 99, 20, 20) < -0.45  # uniform in [-0.5, 0.5)
    elif kind == "two":
        flat[[npix // 3, npix - 2]] = True
    elif kind == "one":
        flat[npix // 2] = True
    elif kind != "empty":
        raise ValueError(kind)
    return flat.reshape(shape)


def window_mask(shape):
    """About 60 % of the pixels in blobs, the top-left 12 x 12 corner empty but for an island of two pixels: no window
    there holds three values, however wide."""
    m, n = shape
    flat = _grid_noise(m * n, 321, 20, 20) < 0.1
    mask = flat.reshape(shape)
    mask[:12, :12] = False
    mask[2, 3] = mask[2, 4] = True
    return mask


def spatial_cases():
    """(name, shape, L, T, d, dtype, mask kind, variant): every combination of shape, levels, frames, d and dtype under
    alternating None / sparse masks; every mask kind and every variant at each shape and dtype."""
    cases = []
    for shape in SHAPES:
        for L in LEVELS:
            for T in FRAMES:
                for d in (0, 1):
                    for dtype in DTYPES:
                        cases.append((shape, L, T, d, dtype, "sparse" if (L + T + d) % 2 else "none", "plain"))
        for dtype in DTYPES:
            for kind in MASKS:
                cases.append((shape, 3, 3, 0, dtype, kind, "plain"))
            for variant in VARIANTS[1:]:
                cases.append((shape, 3, 3, 0, dtype, "all", variant))
                cases.append((shape, 1, 4, 1, dtype, "none", variant))
    seen, out = set(), []
    for c in cases:
        name = "sp_%dx%d_L%d_T%d_d%d_%s_%s_%s" % (c[0] + c[1:])
        if name not in seen:
            seen.add(name)
            out.append((name,) + c)
    return out


def spectral_cases():
    """(name, shape, L, T, d, use_full_fft)."""
    return [("fx_%dx%d_L%d_T%d_d%d_%s" % (shape + (L, T, d, "full" if full else "half")), shape, L, T, d, full)
            for shape in SPECTRAL_SHAPES for (L, T, d) in ((1, 2, 0), (3, 3, 0), (3, 4, 1)) for full in (False, True)]


def window_cases():
    """(name, T, d, sigma, masked)."""
    cases = [("win_T2_d0_s%s_%s" % (sigma, "mask" if masked else "nomask"), 2, 0, sigma, masked)
             for sigma in WINDOW_SIGMAS for masked in (False, True)]
    return cases + [("win_T3_d0_s1.5_mask", 3, 0, 1.5, True), ("win_T3_d1_s4_nomask", 3, 1, 4, False)]


def hermitian_full(half, n):
    """fft2 of a real field from its rfft2 half (..., m, n//2+1): X[r, c] = conj(X[-r, n - c]) for c > n//2."""
    m = half.shape[-2]
    full = np.empty(half.shape[:-1] + (n,), dtype=half.dtype)
    nc = half.shape[-1]
    full[..., :nc] = half
    rows = (-np.arange(m)) % m
    for c in range(nc, n):
        full[..., c] = np.conj(half[..., rows, n - c])
    return full


def spectral_cascade(half, L, T, full, n):
    """(L, T, m, nc) from the stored half spectra of T_max frames: level l takes the frames rolled by l (the levels'
    coefficients differ, nothing new is stored)."""
    frames = half.shape[0]
    out = np.stack([np.stack([half[(t + l) % frames] for t in range(T)]) for l in range(L)])
    return np.ascontiguousarray(hermitian_full(out, n) if full else out)


# ---- the reference's arithmetic -------------------------------------------------------------------------------------

def corrcoef_spectral(X, Y, shape, use_full_fft=False):
    """pysteps/utils/spectral.py:62-76."""
    n = np.real(np.sum(X * np.conj(Y))) - np.real(X[0, 0] * Y[0, 0])
    d1 = np.sum(np.abs(X) ** 2) - np.real(X[0, 0]) ** 2
    d2 = np.sum(np.abs(Y) ** 2) - np.real(Y[0, 0]) ** 2
    if not use_full_fft:
        inner = slice(1, None) if shape[1] % 2 == 1 else slice(1, -1)
        n += np.real(np.sum(X[:, inner] * np.conj(Y[:, inner])))
        d1 += np.sum(np.abs(X[:, inner]) ** 2)
        d2 += np.sum(np.abs(Y[:, inner]) ** 2)
    return n / np.sqrt(d1 * d2)


def moving_window_corrcoef(x, y, sigma, mask):
    """correlation.py:222-271 with the Gaussian window."""
    from scipy.ndimage import gaussian_filter  # noqa: PLC0415

    x, y = x.copy(), y.copy()
    x[~mask] = 0.0
    y[~mask] = 0.0
    maskf = mask.astype(float)
    f = lambda a: gaussian_filter(a, sigma, mode="constant") * sigma**2  # noqa: E731
    n, sx, sy, ssx, ssy, sxy = f(maskf), f(x), f(y), f(x**2), f(y**2), f(x * y)
    with np.errstate(all="ignore"):
        mux, muy = sx / n, sy / n
        stdx = np.sqrt(ssx - 2 * mux * sx + n * mux**2)
        stdy = np.sqrt(ssy - 2 * muy * sy + n * muy**2)
        cov = sxy - muy * sx - mux * sy + n * mux * muy
        ok = np.logical_and(np.logical_and(np.logical_and(stdx > 1e-8, stdy > 1e-8), stdx * stdy > 1e-8), n >= 3)
        corr = np.full(x.shape, np.nan)
        corr[ok] = cov[ok] / (stdx[ok] * stdy[ok])
    return corr


def reference_float64(x, d=0, domain="spatial", x_shape=None, mask=None, use_full_fft=False, window_radius=np.inf):
    """correlation.py:109-130 for input that passed the checks."""
    if d == 1:
        x = np.diff(x, axis=0)
    if domain == "spatial" and mask is None:
        mask = np.ones(x.shape[1:], dtype=bool)
    out = []
    for k in range(x.shape[0] - 1):
        if domain == "spectral":
            out.append(corrcoef_spectral(x[-1], x[-(k + 2)], x_shape, use_full_fft))
        elif window_radius == np.inf:
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")  # an empty or one-pixel selection: NaN, as the callers see it
                out.append(np.corrcoef(x[-1][mask], x[-(k + 2)][mask])[0, 1])
        else:
            out.append(moving_window_corrcoef(x[-1], x[-(k + 2)], window_radius, mask))
    return out


# ---- exact sums, longdouble finish --------------------------------------------------------------------------------

def _wide(frac):
    """A rational as numpy.longdouble (two float64 words: 106 bits before longdouble rounds)."""
    hi = float(frac)
    return np.longdouble(hi) + np.longdouble(float(frac - Fraction(hi)))


def _finish(num, den2):
    """num / sqrt(den2) of rationals in longdouble, rounded to float64 (NaN for den2 <= 0)."""
    if den2 <= 0:
        return float("nan")
    if num == 0:
        return 0.0
    root = np.sqrt(_wide(num * num / den2))
    return float(-root if num < 0 else root)


def integer_series(x, d, grid):
    """The (differenced) series of ``x`` ``(T, npix)`` as Python integers in units of 2^-grid, newest first."""
    rows = [[int(v) for v in (plane.astype(np.float64) * 2.0 ** grid)] for plane in x]
    assert all(float(v) * 2.0 ** -grid == float(w) for v, w in zip(rows[0][:16], x[0][:16]))
    if d == 1:
        rows = [[b - a for a, b in zip(rows[t], rows[t + 1])] for t in range(len(rows) - 1)]
    return rows[::-1]


def exact_sums(x, d, mask, grid):
    """(count, rows) of one level ``(T, ...)``: rows = [S_a, S_aa, then per lag S_b, S_bb, S_ab] as rationals - what
    ``psh_autocorr_sums_dev`` returns as double-double pairs."""
    T = x.shape[0]
    flat = x.reshape(T, -1)
    sel = np.arange(flat.shape[1]) if mask is None else np.flatnonzero(mask.reshape(-1))
    series = integer_series(flat[:, sel], d, grid)
    u, uu = Fraction(1, 1 << grid), Fraction(1, 1 << (2 * grid))
    a = series[0]
    rows = [sum(a) * u, sum(v * v for v in a) * uu]
    for b in series[1:]:
        rows += [sum(b) * u, sum(v * v for v in b) * uu, sum(v * w for v, w in zip(a, b)) * uu]
    return len(sel), rows


def exact_gamma(x, d, mask, dtype):
    """One level's coefficients: integer sums, the finish in longdouble, rounded to float64; NaN for fewer than two
    values or a plane without variance, clipped to [-1, 1] like the rounded result of ``np.corrcoef``."""
    count, rows = exact_sums(x, d, mask, _GRID[dtype])
    out = []
    for k in range((len(rows) - 2) // 3):
        s_a, s_aa, (s_b, s_bb, s_ab) = rows[0], rows[1], rows[2 + 3 * k:5 + 3 * k]
        if count < 2:
            out.append(float("nan"))
            continue
        g = _finish(count * s_ab - s_a * s_b, (count * s_aa - s_a * s_a) * (count * s_bb - s_b * s_b))
        out.append(min(1.0, max(-1.0, g)) if g == g else g)
    return out


def exact_gamma_spectral(x, d, shape, use_full_fft):
    """One level's spectral coefficients ``(T, m, nc)``: every product and sum in rationals (the DC terms as the
    reference writes them, which for a real field's spectrum are the exact ones), the finish in longdouble."""
    if d == 1:
        x = np.diff(x, axis=0)
    nc = x.shape[-1]
    h = np.full(nc, 2)
    h[0] = 1
    if shape[1] % 2 == 0:
        h[-1] = 1
    if use_full_fft:
        h[:] = 1
    weights = [int(v) for v in np.broadcast_to(h, x.shape[1:]).reshape(-1)]
    F = lambda plane: ([Fraction(float(v)) for v in plane.real.reshape(-1)], [Fraction(float(v)) for v in plane.imag.reshape(-1)])  # noqa: E731
    Xr, Xi = F(x[-1])
    d1 = sum(w * (r * r + i * i) for w, r, i in zip(weights, Xr, Xi)) - Xr[0] * Xr[0]
    out = []
    for k in range(x.shape[0] - 1):
        Yr, Yi = F(x[-(k + 2)])
        n = sum(w * (a * b + c * e) for w, a, b, c, e in zip(weights, Xr, Yr, Xi, Yi)) - (Xr[0] * Yr[0] - Xi[0] * Yi[0])
        d2 = sum(w * (r * r + i * i) for w, r, i in zip(weights, Yr, Yi)) - Yr[0] * Yr[0]
        out.append(_finish(n, d1 * d2))
    return out


def parseval_bar(shape, L):
    """How far the coefficient of stored float64 spectra may lie from the exact coefficient of their fields: a
    transform's bins carry eps * log2(m n) of relative error, a coefficient is a ratio of three quadratic forms in
    them (4 x), and the DC term that the forms subtract is 1 + mean^2 / var times what is left (the levels' means are
    1.5 + 2.5 l over a variance of 6)."""
    mean = 1.5 + 2.5 * (L - 1)
    return 4.0 * float(np.finfo(np.float64).eps) * np.log2(shape[0] * shape[1]) * (1.0 + mean * mean / 6.0)


def exact_abs_sums(x, d, mask, grid):
    """The sums of :func:`exact_sums` with every term's absolute value: what an addition's rounding is relative to."""
    T = x.shape[0]
    flat = x.reshape(T, -1)
    sel = np.arange(flat.shape[1]) if mask is None else np.flatnonzero(mask.reshape(-1))
    series = integer_series(flat[:, sel], d, grid)
    u, uu = Fraction(1, 1 << grid), Fraction(1, 1 << (2 * grid))
    a = series[0]
    rows = [sum(abs(v) for v in a) * u, sum(v * v for v in a) * uu]
    for b in series[1:]:
        rows += [sum(abs(v) for v in b) * u, sum(v * v for v in b) * uu, sum(abs(v * w) for v, w in zip(a, b)) * uu]
    return rows


def dd_value(pair):
    """A double-double pair as a rational."""
    return Fraction(float(pair[0])) + Fraction(float(pair[1]))


def max_abs_dev(a, b):
    """Largest absolute difference where both are numbers; the NaN patterns must agree."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(a)
    return float(np.max(np.abs(a[ok] - b[ok]))) if ok.any() else 0.0


# ---- the AR estimate ----------------------------------------------------------------------------------------------

# lag-1, lag-2[, lag-3] coefficients: typical cascade levels, a level near 1, a weak one, a negative lag 1, values the
# adjustments change
AR_GAMMAS = [(0.95, 0.88, 0.8), (0.999, 0.9975, 0.995), (0.31, 0.05, 0.01), (-0.4, 0.3, -0.1), (0.9, 0.5, 0.4), (0.6, 0.9, 0.2),
             (0.8, 0.64, 0.512)]
AR_NONSTATIONARY = (0.5, -0.9)  # Yule-Walker gives phi_2 = -1.53: a root outside the unit circle


def yw_bound(gamma, chain, h=1e-7):
    """Largest row sum of |d phi / d gamma| of ``chain`` (gamma -> phi) by central differences: what a deviation of
    every coefficient by one unit can move a parameter."""
    gamma = np.asarray(gamma, dtype=np.float64)
    cols = []
    for j in range(gamma.size):
        up, down = gamma.copy(), gamma.copy()
        up[j] += h
        down[j] -= h
        cols.append((np.asarray(chain(up)) - np.asarray(chain(down))) / (2 * h))
    return float(np.max(np.sum(np.abs(np.array(cols)), axis=0)))
