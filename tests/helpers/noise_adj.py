"""Cases and a NumPy restatement of pysteps/noise/utils.py ``compute_noise_stddev_adjs`` (test yardstick).

The restatement writes out what the reference's function does with ``decomposition_fft`` and
``generate_noise_2d_fft_filter`` and NumPy's transforms, array operation by array operation, with a ``dtype``
parameter: at float64 it is the reference bit for bit (tests/test_noise_adj_cpu.py holds it to that), at
``numpy.longdouble`` it is the yardstick that says how far the reference's float64 arithmetic is from the numbers it
stands for.  The white noise is the same float64 ``randn`` stream in every precision, widened.
"""

import numpy as np

# shape, cascade levels, seed of the field - the smallest shapes at which the kernels can go wrong
CASES = {
    "p64x64": ((64, 64), 3, 11),      # power of two
    "o67x129": ((67, 129), 4, 12),    # both sides odd: no Nyquist column, plane not a multiple of the wave
    "e96x130": ((96, 130), 5, 13),    # even sides that are no powers of two: Nyquist column present
    "p256x256": ((256, 256), 6, 14),  # more pixels than a reduction block takes in one stride
}
DRY = -15.0  # dB value of a dry pixel = R_thr_2
MASKS = ("wet", "sparse", "all")
# (conditional, num_iter, seed) of the coefficient checks on the "wet" mask; the other two masks: num_iter 3, seed 0
COMBOS = [(c, k, s) for c in (True, False) for k in (1, 3, 20) for s in (0, 42)]
MASK_COMBOS = [(c, 3, 0) for c in (True, False)]


def field(shape, seed, wet=0.35):
    """A rain-like dB field as float32: smooth cells above -10 dB over a dry background of -15 dB, about ``wet`` of
    the pixels wet."""
    from scipy.ndimage import gaussian_filter  # noqa: PLC0415

    m, n = shape
    rng = np.random.default_rng(seed)
    g = gaussian_filter(rng.standard_normal((m, n)), max(min(m, n) / 24.0, 1.5), mode="wrap")
    g = (g - g.mean()) / g.std()
    cut = np.quantile(g, 1.0 - wet)
    texture = gaussian_filter(rng.standard_normal((m, n)), 1.0, mode="wrap")
    db = np.where(g > cut, -10.0 + 14.0 * (g - cut) + 2.0 * np.abs(texture), DRY)
    return db.astype(np.float32)


def thresholds(R, mask):
    """(R_thr_1, R_thr_2) of a mask kind: "wet" - the rain / no-rain threshold, about 35 % of the pixels; "sparse" - a
    threshold that leaves 40 pixels, less than one wave; "all" - a threshold below the minimum."""
    R = np.asarray(R, dtype=np.float64)
    if mask == "wet":
        return -10.0, DRY
    if mask == "sparse":
        return float(np.sort(R, axis=None)[-40]), DRY
    if mask == "all":
        return DRY - 5.0, DRY
    raise ValueError(mask)


def filters(pysteps, R, levels):
    """(band-pass filter, noise filter) of the reference for a float64 field."""
    from pysteps.cascade.bandpass_filters import filter_gaussian  # noqa: PLC0415
    from pysteps.noise.fftgenerators import initialize_nonparam_2d_fft_filter  # noqa: PLC0415

    return filter_gaussian(R.shape, levels), initialize_nonparam_2d_fft_filter(R)


def seed_chain(seed, num_iter):
    """The reference's chain of generators (utils.py:103-106)."""
    randstates = []
    for _ in range(num_iter):
        rs = np.random.RandomState(seed=seed)
        randstates.append(rs)
        seed = rs.randint(0, high=1e9)
    return randstates


def level_moments(x, weights, mask, dtype):
    """decomposition.py:205-234 for a spatial field: (means, stds) of the levels (over the mask if there is one)."""
    shape = x.shape
    spectrum = np.fft.rfft2(x)
    means, stds = [], []
    for k in range(weights.shape[0]):
        level = np.fft.irfft2(spectrum * weights[k, :, :], s=shape)
        sel = level[mask] if mask is not None else level
        means.append(np.mean(sel))
        stds.append(np.std(sel))
    return means, stds


def filtered_noise(randstate, filt, shape, dtype):
    """fftgenerators.py:400-433 (spatial domain, half-spectrum filter)."""
    N = randstate.randn(shape[0], shape[1]).astype(dtype)
    fN = np.fft.rfft2(N)
    fN *= filt
    N = np.array(np.fft.irfft2(fN, s=shape))
    return (N - N.mean()) / N.std()


def prepared(N, MASK, sigma, mu, R_thr_2):
    """utils.py:113-118."""
    N = N / np.std(N) * sigma + mu
    N[~MASK] = R_thr_2
    N -= mu
    return N


def restated(R, R_thr_1, R_thr_2, weights, filt, num_iter, conditional=True, seed=None, dtype=np.float64):
    """compute_noise_stddev_adjs (utils.py:83-135) with every array in ``dtype``."""
    R = np.asarray(R).astype(dtype)
    weights = np.asarray(weights).astype(dtype)
    filt = np.asarray(filt).astype(dtype)
    MASK = R >= R_thr_1
    R[~np.isfinite(R)] = R_thr_2
    R[~MASK] = R_thr_2
    if not conditional:
        mu, sigma = np.mean(R), np.std(R)
    else:
        mu, sigma = np.mean(R[MASK]), np.std(R[MASK])
    R -= mu
    MASK_ = MASK if conditional else None
    stds_R = level_moments(R, weights, MASK_, dtype)[1]
    N_stds = []
    for rs in seed_chain(seed, num_iter):
        N = prepared(filtered_noise(rs, filt, R.shape, dtype), MASK, sigma, mu, R_thr_2)
        N_stds.append(level_moments(N, weights, MASK_, dtype)[1])
    return stds_R / np.mean(np.vstack(N_stds), axis=0)


def key(name, mask, conditional, num_iter, seed):
    return "%s__%s__%s__k%d__s%d" % (name, mask, "cond" if conditional else "uncond", num_iter, seed)


def all_keys():
    out = []
    for name in CASES:
        out += [(name, "wet") + combo for combo in COMBOS]
        out += [(name, mask) + combo for mask in ("sparse", "all") for combo in MASK_COMBOS]
    return out


def rel_dev(got, want):
    """Largest relative difference per coefficient."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    return float(np.max(np.abs(got - want) / np.abs(want)))
