"""Gaussian band-pass filters for the FFT cascade (restates pysteps/cascade/bandpass_filters.py ``filter_gaussian``).

The ANVIL nowcast (``nowcasts/anvil.py``) builds its cascade with these weights and must not need pysteps.  The
weights are evaluated with the same NumPy operations in the same order as the reference, so they are the same
doubles: log-spaced centres ``q**k`` with ``q = (l/2)**(1/n)``, one Gaussian in ``log_q(wavenumber)`` per band,
normalised so that the bands sum to one at every wavenumber, the mean (wavenumber 0) in the first band only.
"""

import numpy as np

__all__ = ["filter_gaussian"]


def _log_q(x, log_q):
    """log_q(x) with log_q(0) = 0, for an array or a scalar wavenumber."""
    if np.ndim(x) == 0:
        return 0.0 if x == 0.0 else np.log(x) / log_q
    out = np.empty(x.shape)
    out[x == 0] = 0.0
    pos = x > 0
    out[pos] = np.log(x[pos]) / log_q
    return out


def _band_functions(length, n, gauss_scale):
    """The n weight functions of the bands and their central wavenumbers."""
    q = pow(0.5 * length, 1.0 / n)
    log_q = np.log(q)
    centres = [0.5 * (pow(q, k - 1) + pow(q, k)) for k in range(1, n + 1)]
    two_s2 = 2.0 * gauss_scale**2.0

    def band(centre_log):
        def weight(x):
            d = _log_q(x, log_q) - centre_log
            return np.exp(-(d**2.0) / two_s2)

        return weight

    return [band(_log_q(c, log_q)) for c in centres], centres


def filter_gaussian(shape, n, gauss_scale=0.5, d=1.0, normalize=True, return_weight_funcs=False, include_mean=True):
    """Gaussian band-pass filters in a logarithmic frequency scale.  Parameters and the returned dictionary as in
    the reference (``weights_1d``, ``weights_2d`` (n, height, width // 2 + 1), ``shape``, ``central_wavenumbers``,
    ``central_freqs``, optionally ``weight_funcs``)."""
    if n < 3:
        raise ValueError("n must be greater than 2")
    try:
        height, width = shape
    except TypeError:
        height, width = (shape, shape)
    longest = max(width, height)

    # wavenumber of every bin of the half spectrum: rows in FFT order, columns 0 .. width // 2
    half_h = int(height / 2)
    rows = np.arange(-half_h, half_h + 1) if height % 2 == 1 else np.arange(-half_h, half_h)
    cols = np.arange(int(width / 2) + 1)
    ky, kx = rows[:, None], cols[None, :]
    shift = half_h if height % 2 == 0 else half_h + 1
    radius_2d = np.roll(np.sqrt(kx * kx + ky * ky), shift, axis=0)
    r_max = int(longest / 2) + 1
    radius_1d = np.arange(r_max)

    funcs, centres = _band_functions(longest, n, gauss_scale)
    w1 = np.empty((n, r_max))
    w2 = np.empty((n, height, int(width / 2) + 1))
    for i, f in enumerate(funcs):
        w1[i, :] = f(radius_1d)
        w2[i, :, :] = f(radius_2d)
    if normalize:
        s1 = np.sum(w1, axis=0)
        s2 = np.sum(w2, axis=0)
        for k in range(n):
            w1[k, :] /= s1
            w2[k, :, :] /= s2
    for i in range(n):
        mean_weight = 1.0 if (i == 0 and include_mean) else 0.0
        w1[i, 0] = mean_weight
        w2[i, 0, 0] = mean_weight

    out = {"weights_1d": w1, "weights_2d": w2, "shape": shape}
    wavenumbers = np.array(centres)
    out["central_wavenumbers"] = wavenumbers
    freqs = 1.0 * wavenumbers / longest
    freqs[0] = 1.0 / longest
    freqs[-1] = 0.5
    out["central_freqs"] = 1.0 * d * freqs
    if return_weight_funcs:
        out["weight_funcs"] = funcs
    return out
