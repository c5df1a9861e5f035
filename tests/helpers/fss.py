"""NumPy integer restatement of the sums behind pysteps/verification/spatialscores.py ``fss_accum`` (test yardstick),
and the generators of the test fields.

The reference thresholds both fields (non-finite values are set to ``thr - 1``, so they count as "below"), averages the
0/1 maps with ``scipy.ndimage.uniform_filter(size=s, mode="constant", cval=0)`` and sums ``S_f**2``, ``S_f * S_o`` and
``S_o**2``.  ``S = c / s**2`` with ``c`` the number of ones in the window of pixel ``(y, x)``: rows
``y - s // 2 .. y - s // 2 + s - 1`` and the same columns, clipped to the image.  Here ``c`` is counted in int64 from a
2-d cumulative sum and its four clipped corners, and the three sums are returned as Python integers: ``sum(c_f**2)``,
``sum(c_f * c_o)``, ``sum(c_o**2)``; the reference's sums are these over ``s**4``.
"""

import numpy as np

SCALES = [1, 2, 3, 8, 16, 33, 64, 128, 255]
THRESHOLDS = [0.5, 0.7, 4.0]  # Python floats; 0.7 lies in the rounding gap of float32(0.7), a value the fields hold


def indicator(X, thr):
    """finite and ``>= thr``, compared as NumPy compares an array of X's dtype with ``thr``."""
    X = np.asarray(X)
    out = np.zeros(X.shape, dtype=bool)
    fin = np.isfinite(X)
    out[fin] = X[fin] >= thr
    return out


def window(scale):
    return int(scale) if scale > 1 else 1


def window_counts(binary, scale):
    """int64 (m, n): the number of ones of ``binary`` in the window of every pixel."""
    m, n = binary.shape
    s = window(scale)
    C = np.zeros((m + 1, n + 1), dtype=np.int64)
    np.cumsum(np.cumsum(binary, axis=0, dtype=np.int64), axis=1, out=C[1:, 1:])
    r0 = np.clip(np.arange(m) - s // 2, 0, m)
    r1 = np.clip(np.arange(m) - s // 2 + s, 0, m)
    c0 = np.clip(np.arange(n) - s // 2, 0, n)
    c1 = np.clip(np.arange(n) - s // 2 + s, 0, n)
    top, bottom = C[r0], C[r1]
    return bottom[:, c1] - top[:, c1] - bottom[:, c0] + top[:, c0]


def sums(X_f, X_o, thr, scale):
    """(sum c_f^2, sum c_f c_o, sum c_o^2) as Python integers."""
    cf = window_counts(indicator(X_f, thr), scale)
    co = window_counts(indicator(X_o, thr), scale)
    return int((cf * cf).sum()), int((cf * co).sum()), int((co * co).sum())


def sums_table(X_f, X_o, thrs, scales):
    """Object array (K, nthr, nsc, 3) of Python integers for a stack (or one field) against a plane or a stack."""
    X_f, X_o = np.asarray(X_f), np.asarray(X_o)
    stack = X_f[None] if X_f.ndim == 2 else X_f
    out = np.empty((stack.shape[0], len(thrs), len(scales), 3), dtype=object)
    for k in range(stack.shape[0]):
        obs = X_o if X_o.ndim == 2 else X_o[k]
        for i, thr in enumerate(thrs):
            bf, bo = indicator(stack[k], thr), indicator(obs, thr)
            for j, scale in enumerate(scales):
                cf, co = window_counts(bf, scale), window_counts(bo, scale)
                out[k, i, j] = [int((cf * cf).sum()), int((cf * co).sum()), int((co * co).sum())]
    return out[0] if X_f.ndim == 2 else out


def as_float_sums(counts, scale):
    """The float64 sums an FSS object holds: exact integers, one correctly rounded division each."""
    w = window(scale)
    return [np.float64(int(c) / w**4) for c in counts]


def score(counts, scale):
    """The FSS of integer sums, by the reference's formula (NaN for an all-dry pair, without a warning)."""
    ff, fo, oo = as_float_sums(counts, scale)
    with np.errstate(invalid="ignore"):
        return np.float64(1.0) - (ff - 2.0 * fo + oo) / (ff + oo)


def field(m, n, seed, dtype=np.float32, wet=0.35, specials=True):
    """A rain-like field: smooth cells over a dry background, intensities in steps of 0.5, some pixels exactly
    float32(0.7); with ``specials`` a NaN speckle, a +inf block and a -inf block."""
    from scipy.ndimage import gaussian_filter  # noqa: PLC0415

    rng = np.random.default_rng(seed)
    g = gaussian_filter(rng.standard_normal((m, n)), 9.0, mode="wrap")
    g = (g - g.mean()) / g.std()
    cut = np.quantile(g, 1.0 - wet)
    x = (np.round(np.maximum(g - cut, 0.0) * 12.0) / 2.0).astype(np.float32)
    x[(rng.random((m, n)) < 0.01) & (x > 0)] = np.float32(0.7)
    if specials:
        x[rng.random((m, n)) < 0.001] = np.nan
        y, c = m // 3, n // 4
        x[y:y + 9, c:c + 13] = np.inf
        x[m - y:m - y + 7, n - c:n - c + 11] = -np.inf
    return x.astype(dtype)


def pair(m, n, seed, dtype=np.float32):
    """(forecast, observation): the observation is the forecast displaced, mixed with cells of its own."""
    f = field(m, n, seed, np.float32)
    other = field(m, n, seed + 1000, np.float32, wet=0.15, specials=False)
    o = np.maximum(np.roll(np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0), (5, -9), axis=(0, 1)), other)
    rng = np.random.default_rng(seed + 2000)
    o[rng.random((m, n)) < 0.001] = np.nan
    o[m // 2:m // 2 + 5, n // 2:n // 2 + 6] = np.inf
    return f.astype(dtype), o.astype(dtype)
