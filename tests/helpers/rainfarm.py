"""RainFARM test material (tests/test_rainfarm_*.py, tools/make_golden_rainfarm.py): the case list, the field
generator and a restatement of the reference's plain (no spectral fusion) pipeline with the uniforms as an argument.

``pipeline(..., dtype=np.float64)`` makes the same NumPy / SciPy calls as pysteps/downscaling/rainfarm.py, in its order.
``dtype=np.longdouble`` is the yardstick: the same formulas in extended precision (numpy >= 2 transforms in the input's
precision, as helpers/fft_pointwise.py relies on), the wavenumbers exact (k ds / M), the convolution a direct sum.
"""

import os

import numpy as np

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "rainfarm_reference.npz")
FULL_LIMIT = 64 * 128  # outputs up to this many pixels are stored whole
BAR_FACTOR = 5.0

# name, low-res shape, ds, kernel, alpha (None: estimated), seed
CASES = [
    ("pow2_16x32_ds4", (16, 32), 4, None, None, 101),
    ("chirp_20x27_ds3_gauss", (20, 27), 3, "gaussian", None, 102),
    ("r5_24x40_ds8_tophat", (24, 40), 8, "tophat", 2.5, 103),
    ("border_4x5_ds16_gauss", (4, 5), 16, "gaussian", 1.7, 104),
    ("odd_33x17_ds1_tophat", (33, 17), 1, "tophat", None, 105),
    ("flat_32x32_ds2_uniform", (32, 32), 2, "uniform", 0.0, 106),
    ("large_128x128_ds8_gauss", (128, 128), 8, "gaussian", None, 107),
]
THRESHOLD_CASES = ("pow2_16x32_ds4", "r5_24x40_ds8_tophat")
THRESHOLD_SKIP_SHARE = 1e-3  # at most this share of a case's pixels may lie within the bar of a threshold


def stride_for(shape):
    """Rows / columns kept of a stored output: every one, every 3rd or every 7th (coprime to the factors used)."""
    px = int(shape[0]) * int(shape[1])
    return 1 if px <= FULL_LIMIT else (3 if px <= 300000 else 7)


def field(shape, seed):
    """A seeded rain-like field: smooth log-normal cells over a dry background, values in 1/8 steps."""
    m, n = shape
    rng = np.random.RandomState(seed)
    white = rng.randn(m, n)
    ky = np.fft.fftfreq(m)[:, None]
    kx = np.fft.fftfreq(n)[None, :]
    k = np.sqrt(ky**2 + kx**2)
    k[0, 0] = 1.0
    smooth = np.fft.ifft2(np.fft.fft2(white) * k**-1.2).real
    smooth /= smooth.std()
    rain = np.exp(1.2 * smooth) * 2.0
    rain[smooth < -0.4] = 0.0
    return np.round(rain * 8.0) / 8.0


def kernel_radius(ds):
    return int(round(ds / np.sqrt(np.pi)))


def make_kernel(kernel_type, ds, dtype=np.float64):
    r = kernel_radius(ds)
    if kernel_type == "gaussian":
        sigma = dtype(ds) / 2
        x = np.arange(-r, r + 1).astype(dtype)
        k1 = np.exp(-0.5 / (sigma * sigma) * x**2)
        k2 = np.outer(k1, k1)
        return k2 / k2.sum()
    mx, my = np.mgrid[-r : r + 0.01, -r : r + 0.01]
    top = ((mx**2 + my**2) <= r**2).astype(dtype)
    return top / top.sum()


def convolve_same_direct(x, kernel):
    """Zero-padded ``mode="same"`` convolution as a direct sum (the kernels are symmetric under both flips)."""
    r = (kernel.shape[0] - 1) // 2
    M, N = x.shape
    pad = np.zeros((M + 2 * r, N + 2 * r), dtype=x.dtype)
    pad[r : r + M, r : r + N] = x
    out = np.zeros_like(x)
    c = kernel.sum(axis=0)  # a normalised outer product c c^T (the Gaussian) is summed along one axis at a time
    if np.abs(np.outer(c, c) - kernel).max() <= 8 * np.finfo(kernel.dtype).eps * kernel.max():
        rows = np.zeros((M + 2 * r, N), dtype=x.dtype)
        for dx in range(2 * r + 1):
            rows += c[dx] * pad[:, dx : dx + N]
        for dy in range(2 * r + 1):
            out += c[dy] * rows[dy : dy + M]
        return out
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            w = kernel[dy, dx]
            if w != 0:
                out += w * pad[dy : dy + M, dx : dx + N]
    return out


def balanced_average(x, kernel, direct, weight=None):
    """``_balanced_spatial_average`` of an all-finite plane; ``weight``: the direct convolution of the all-ones mask."""
    if direct:
        return convolve_same_direct(x, kernel) / (convolve_same_direct(np.ones_like(x), kernel) if weight is None else weight)
    from scipy.signal import convolve

    out = convolve(x.copy(), kernel, mode="same")
    out /= convolve(np.isfinite(x), kernel, mode="same")
    return out


def freq_array(shape, ds, dtype=np.float64):
    if dtype == np.float64:
        fi = np.fft.fftfreq(shape[0] * ds, d=1 / ds)
        fj = np.fft.fftfreq(shape[1] * ds, d=1 / ds)
    else:
        M, N = shape[0] * ds, shape[1] * ds
        fi = (np.fft.fftfreq(M) * M).round().astype(dtype) * ds / M
        fj = (np.fft.fftfreq(N) * N).round().astype(dtype) * ds / N
    return np.sqrt(fi[:, None] ** 2 + fj[None, :] ** 2)


_PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def noise_field(u, alpha, lowres_shape, ds, dtype=np.float64):
    """``_compute_noise_field`` with the uniforms given."""
    f = freq_array(lowres_shape, ds, dtype)
    if dtype == np.float64:
        white = np.exp(complex(0, 1) * 2 * np.pi * u)
        with np.errstate(all="ignore"):
            z = white * np.sqrt(f**-alpha)
        z[0, 0] = 0
        return np.fft.ifft2(z).real
    a = 2 * _PI_LD * u.astype(dtype)
    f[0, 0] = 1
    amp = np.sqrt(f ** (-dtype(alpha)))
    z = (np.cos(a) + 1j * np.sin(a)) * amp
    z[0, 0] = 0
    return np.fft.ifft2(z).real


def aggregate(x, ds):
    M, N = x.shape
    a = x.swapaxes(0, 0).reshape(M // ds, ds, -1).mean(axis=1).reshape(M // ds, N)
    b = a.swapaxes(1, 0).reshape(N // ds, ds, -1).mean(axis=1).reshape(N // ds, M // ds).swapaxes(1, 0)
    return b


def finish(precip, noise, ds, kernel_type, dtype=np.float64):
    """Everything after the transform, without the threshold.  Returns (field, max |noise / std|)."""
    direct = dtype != np.float64
    noise = noise.astype(dtype) / noise.astype(dtype).std()
    g = float(np.abs(noise).max())
    e = np.exp(noise)
    low = aggregate(e, ds)
    ones = np.ones((ds, ds), dtype=dtype)
    p_exp = np.kron(np.asarray(precip).astype(dtype), ones)
    l_exp = np.kron(low, ones)
    if kernel_type:
        kernel = make_kernel(kernel_type, ds, dtype)
        weight = convolve_same_direct(np.ones_like(p_exp), kernel) if direct else None
        p_exp = balanced_average(p_exp, kernel, direct, weight)
        l_exp = balanced_average(l_exp, kernel, direct, weight)
    return e * (p_exp / l_exp), g


def pipeline(precip, u, ds, alpha, kernel_type, dtype=np.float64):
    noise = noise_field(u, alpha, np.shape(precip), ds, dtype)
    return finish(precip, noise, ds, kernel_type, dtype)[0]


def log_slope(log_k, log_ps):
    lk_min, lk_max = log_k.min(), log_k.max()
    lk_range = lk_max - lk_min
    lk_min += (1 / 6) * lk_range
    lk_max -= (1 / 6) * lk_range
    sel = (lk_min <= log_k) & (log_k <= lk_max)
    return -np.polyfit(log_k[sel], log_ps[sel], 1)[0]


def estimate_alpha(precip, fft2=np.fft.fft2, dtype=np.float64):
    """``_estimate_alpha`` with the transform as an argument; ``dtype=np.longdouble``: transform, logarithms and the
    least-squares line (closed form) in extended precision."""
    precip = np.asarray(precip).astype(dtype)
    k = freq_array(precip.shape, 1, np.float64).astype(dtype)
    with np.errstate(all="ignore"):
        lp = np.log(np.abs(fft2(precip)) ** 2)
    valid = (k != 0) & np.isfinite(lp)
    if dtype == np.float64:
        return log_slope(np.log(k[valid]), lp[valid])
    lk, ps = np.log(k[valid]), lp[valid]
    lo, hi = lk.min(), lk.max()
    rng = hi - lo
    sel = (lo + rng / 6 <= lk) & (lk <= hi - rng / 6)
    x, y = lk[sel], ps[sel]
    xm, ym = x.mean(), y.mean()
    return float(-((x - xm) * (y - ym)).sum() / ((x - xm) ** 2).sum())


def draw(seed, shape):
    """The uniforms the reference draws for this seed."""
    return np.random.RandomState(seed).rand(*shape)


def scaled_diff(got, want):
    """max |got - want| / max |want|: the scale every field comparison uses."""
    want = np.asarray(want)
    err = np.abs(np.asarray(got).astype(np.longdouble) - want.astype(np.longdouble))
    err = np.where(np.isfinite(err), err, np.inf)
    return float(err.max() / np.abs(want).max())


def load_golden():
    return np.load(GOLDEN_FILE, allow_pickle=False)
