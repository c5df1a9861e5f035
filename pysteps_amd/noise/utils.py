"""The noise standard-deviation adjustment of STEPS on the GPU (mirror of pysteps/noise/utils.py:24-135,
``compute_noise_stddev_adjs``) - what ``nowcasts.steps(noise_stddev_adj="auto")`` runs before its main loop.

The reference draws ``num_iter`` white-noise fields from a chain of generators, filters each, rescales it to the
observed field's statistics, masks it, decomposes it into the cascade and compares the levels' standard deviations
with those of the observed field.  Here the host keeps what is cheap and order-dependent - the seed chain, the
hand-over of the generator states, the final division - and everything else stays in HBM:

* all realisations' white noise in one draw (:class:`~pysteps_amd.noise.randstate.DeviceRandomStates`),
* the noise filter per realisation (``psh_noise_filter_dev``),
* rescale-and-mask on a batch (``psh_noise_adj_prepare_dev``, csrc/noise_adj.hip),
* ``conditional=True``: the cascade levels (``psh_cascade_decompose_levels_dev``) and their moments over the wet
  pixels (``psh_masked_moments_dev``); ``conditional=False``: one forward transform and the level moments read off
  the spectrum (``psh_spectrum_level_moments_dev``) - no inverse transform per level.

The observed field goes up once; ``2 L`` doubles per realisation come down.  Calls the device path does not take
(see :func:`_decline_reason`) run the reference's function with a ``RuntimeWarning`` that says why.
"""

import warnings

import numpy as np

from .. import _lib
from .._reference import _is_fn, lookup
from ..cascade.decomposition import _device_weights, _self_conjugate_columns_symmetric
from ..device import DeviceArray
from ..utils import fft as hip_fft
from .randstate import DeviceRandomStates

__all__ = ["compute_noise_stddev_adjs"]

MAX_LEVELS = 16
# device memory the realisations of one batch may take (filtered field + cascade levels or spectrum); the result
# does not depend on it
BATCH_BYTES = 8 << 30
# planes that share one read of the mask in psh_masked_moments_dev (1 or 4; same bits).  Measured at 4096^2, 8 levels
# (tools/noise_adj_quick.py): 0.239 ms with one plane per block, 0.262 ms with four - the byte saved per pixel and
# plane is less than what the fourfold accumulators cost, so every plane reads the mask itself
PLANES_PER_BLOCK = 1



def _seed_chain(seed, num_iter):
    """utils.py:103-106, as the reference writes it: one generator per realisation, each seeded by a draw of the one
    before."""
    randstates = []
    for _ in range(num_iter):
        rs = np.random.RandomState(seed=seed)
        randstates.append(rs)
        seed = rs.randint(0, high=1e9)
    return randstates


def _decline_reason(R, R_thr_1, F, decomp_method, noise_filter, noise_generator, num_iter, conditional):
    """Why the device path does not take this call (None: it does).  Needs no device."""
    resident = isinstance(R, DeviceArray)
    if not resident and not isinstance(R, np.ndarray):
        return "R is neither a NumPy array nor a DeviceArray"
    if len(R.shape) != 2:
        return "R is not two-dimensional"
    if np.dtype(R.dtype) != np.float64:
        return "R is %s, the device path is float64 (the reference carries single precision through)" % np.dtype(R.dtype)
    shape = tuple(int(s) for s in R.shape)
    if not hip_fft.supported_shape(shape):
        return "the HIP transforms do not take the shape %s" % (shape,)
    if not _is_fn(decomp_method, "cascade.decomposition", "decomposition_fft"):
        return "decomp_method is not decomposition_fft"
    if not _is_fn(noise_generator, "noise.fftgenerators", "generate_noise_2d_fft_filter"):
        return "noise_generator is not generate_noise_2d_fft_filter"
    m, n = shape
    try:
        field = noise_filter["field"]
        if noise_filter["use_full_fft"]:
            return "the noise filter is a full-spectrum one (use_full_fft)"
        if tuple(noise_filter["input_shape"]) != shape:
            return "the noise filter was made for another shape"
    except (KeyError, TypeError):
        return "noise_filter is not a filter dictionary of the FFT generators"
    if not isinstance(field, np.ndarray) or field.shape != (m, n // 2 + 1) or np.iscomplexobj(field):
        return "the noise filter's field is not a real (m, n//2+1) array"
    if not np.all(np.isfinite(field)):
        return "the noise filter's field holds non-finite values"
    try:
        weights = F["weights_2d"]
    except (KeyError, TypeError):
        return "F is not a band-pass filter dictionary"
    if not isinstance(weights, np.ndarray) or weights.ndim != 3 or weights.shape[1:] != (m, n // 2 + 1):
        return "the band-pass weights are not (levels, m, n//2+1)"
    if not 1 <= weights.shape[0] <= MAX_LEVELS:
        return "more than %d cascade levels" % MAX_LEVELS
    if "weights_1d" in F and len(F["weights_1d"]) != weights.shape[0]:
        return "weights_1d and weights_2d of the band-pass filter disagree"
    if not isinstance(num_iter, (int, np.integer)) or num_iter < 1:
        return "num_iter < 1"
    if conditional and not resident and int(np.count_nonzero(R >= R_thr_1)) < 2:
        return "fewer than two wet pixels to condition on"
    return None


def _to_reference(reason, R, args, kwargs):
    ref = lookup("noise.utils", "compute_noise_stddev_adjs", compute_noise_stddev_adjs)
    if ref is None:
        raise NotImplementedError("pysteps_amd compute_noise_stddev_adjs: %s, and pysteps is not importable for the "
                                  "reference's function" % reason)
    warnings.warn("pysteps_amd compute_noise_stddev_adjs: %s - running the reference's function" % reason, RuntimeWarning,
                  stacklevel=3)
    if isinstance(R, DeviceArray):
        R = R.to_host()
    return ref(R, *args, **kwargs)


def _host_pairs(dev, count):
    """``count`` (mean, std) pairs of a device array as a (count, 2) NumPy array (waits)."""
    out = np.empty((count, 2), dtype=np.float64)
    _lib.check(_lib.lib().psh_memcpy_d2h(out.ctypes.data, dev.ptr, out.nbytes), "psh_memcpy_d2h")
    return out


def mask_count(mask):
    """Number of set bytes of a uint8 DeviceArray, as a device word (uint64 DeviceArray of one element)."""
    count = DeviceArray((1,), np.uint64)
    _lib.check(_lib.lib().psh_mask_count_dev(mask.ptr, mask.size, count.ptr), "psh_mask_count_dev")
    return count


def masked_moments(planes, mask, count=None, planes_per_block=None):
    """``(np.mean(x[mask]), np.std(x[mask]))`` of every plane of a float64 DeviceArray ``(nplanes, m, n)`` (or one
    plane ``(m, n)``) over a uint8 DeviceArray mask ``(m, n)``: a float64 DeviceArray ``(nplanes, 2)``.  ``count``:
    the mask's :func:`mask_count`, taken here if not given."""
    nplanes = 1 if planes.ndim == 2 else int(planes.shape[0])
    plane = int(mask.size)
    if planes.dtype != np.float64 or mask.dtype != np.uint8 or planes.size != nplanes * plane:
        raise ValueError("masked_moments: float64 planes and a uint8 mask of one plane's shape")
    if count is None:
        count = mask_count(mask)
    stats = DeviceArray((nplanes, 2), np.float64)
    _lib.check(_lib.lib().psh_masked_moments_dev(planes.ptr, nplanes, plane, mask.ptr, count.ptr,
                                                 PLANES_PER_BLOCK if planes_per_block is None else int(planes_per_block), stats.ptr),
               "psh_masked_moments_dev")
    return stats


def spectrum_level_moments(spectra, weights, shape):
    """(mean, std) of every cascade level of the fields whose rfft2 half spectra are ``spectra`` (complex128
    DeviceArray ``(nspec, m, n//2+1)`` or one spectrum), read off the spectra: float64 DeviceArray ``(nspec, L, 2)``."""
    m, n = shape
    nspec = 1 if spectra.ndim == 2 else int(spectra.shape[0])
    L = int(weights.shape[0])
    stats = DeviceArray((nspec, L, 2), np.float64)
    _lib.check(_lib.lib().psh_spectrum_level_moments_dev(spectra.ptr, nspec, weights.ptr, L, m, n, stats.ptr),
               "psh_spectrum_level_moments_dev")
    return stats


def prepare(fields, mask, sigma, mu, R_thr_2, stats_out=None):
    """utils.py:113-118 in place on a float64 DeviceArray ``(nbatch, m, n)`` of filtered noise fields."""
    nbatch = int(fields.shape[0])
    _lib.check(_lib.lib().psh_noise_adj_prepare_dev(fields.ptr, nbatch, int(mask.size), mask.ptr, float(sigma), float(mu),
                                                    float(R_thr_2), stats_out.ptr if stats_out is not None else None),
               "psh_noise_adj_prepare_dev")
    return fields


def _per_realisation_bytes(m, n, levels, spectral):
    """Device memory one realisation of a batch takes: its field and its spectrum or its cascade levels."""
    return m * n * 8 + (m * (n // 2 + 1) * 16 if spectral else levels * m * n * 8)


class _Chain:
    """The device state of one call: mask, counts, weights and the two routes to the level statistics."""

    def __init__(self, shape, weights, conditional, spectral):
        self.lib = _lib.lib()
        self.m, self.n = shape
        self.plane = self.m * self.n
        self.L = int(weights.shape[0])
        self.weights = _device_weights(weights)
        self.conditional = conditional
        self.spectral = spectral  # unconditional statistics off the spectrum
        self.mask = DeviceArray(shape, np.uint8)  # R >= R_thr_1
        self.stat_mask = None  # the pixels the level statistics are taken over (spatial routes)
        self.stat_count = None

    def level_stats(self, fields, nbatch):
        """(nbatch, L, 2) host array of the (mean, std) of the cascade levels of ``nbatch`` centred fields."""
        m, n, L = self.m, self.n, self.L
        if self.spectral:
            spectra = DeviceArray((nbatch, m, n // 2 + 1), np.complex128)
            for j in range(nbatch):
                _lib.check(self.lib.psh_fft_rfft2_dev(fields.ptr + j * self.plane * 8, m, n, spectra.view(j).ptr), "psh_fft_rfft2_dev")
            stats = spectrum_level_moments(spectra, self.weights, (m, n))
        else:
            levels = DeviceArray((nbatch * L, m, n), np.float64)
            for j in range(nbatch):
                _lib.check(self.lib.psh_cascade_decompose_levels_dev(fields.ptr + j * self.plane * 8, self.weights.ptr, L, m, n,
                                                                     levels.ptr + j * L * self.plane * 8),
                           "psh_cascade_decompose_levels_dev")
            stats = masked_moments(levels, self.stat_mask, self.stat_count)
        return _host_pairs(stats, nbatch * L).reshape(nbatch, L, 2)


def compute_noise_stddev_adjs(R, R_thr_1, R_thr_2, F, decomp_method, noise_filter, noise_generator, num_iter,
                              conditional=True, num_workers=1, seed=None, *, _batch_bytes=None, _randstates_out=None):
    """Apply a scale-dependent adjustment factor to the noise fields used in STEPS (reference:
    pysteps/noise/utils.py:24-135; parameters as documented there).  Returns a float64 array with one coefficient
    per cascade level.  ``R`` may be a float64 :class:`~pysteps_amd.device.DeviceArray`; it is not modified.
    ``num_workers`` is accepted and ignored on the device path (the realisations are batched on one device).

    ``_batch_bytes`` (tests): device memory one batch of realisations may take instead of :data:`BATCH_BYTES` - the
    result is the same bit for bit; ``_randstates_out`` (tests): a list that receives the chain's generators in the
    states the device left them in."""
    ref_args = (R_thr_1, R_thr_2, F, decomp_method, noise_filter, noise_generator, num_iter)
    ref_kwargs = dict(conditional=conditional, num_workers=num_workers, seed=seed)
    reason = _decline_reason(R, R_thr_1, F, decomp_method, noise_filter, noise_generator, num_iter, conditional)
    if reason is not None:
        return _to_reference(reason, R, ref_args, ref_kwargs)

    lib = _lib.lib()
    m, n = (int(s) for s in R.shape)
    plane = m * n
    weights = F["weights_2d"]
    L = int(weights.shape[0])
    conditional = bool(conditional)
    spectral = not conditional and _self_conjugate_columns_symmetric(weights, n)
    chain = _Chain((m, n), weights, conditional, spectral)

    # utils.py:83-92 - the observed field goes up once
    d_R = R if isinstance(R, DeviceArray) else DeviceArray.from_host(np.ascontiguousarray(R))
    clean = DeviceArray((m, n), np.float64)
    _lib.check(lib.psh_noise_adj_observed_dev(d_R.ptr, plane, float(R_thr_1), float(R_thr_2), chain.mask.ptr, clean.ptr),
               "psh_noise_adj_observed_dev")
    if conditional:
        chain.stat_mask = chain.mask
    else:  # np.mean(R), np.std(R), and the levels' statistics where the spectral route is not taken: every pixel
        chain.stat_mask = DeviceArray((m, n), np.uint8).fill_bytes(1)
    chain.stat_count = mask_count(chain.stat_mask)
    wet = np.empty(1, dtype=np.uint64)
    _lib.check(lib.psh_memcpy_d2h(wet.ctypes.data, chain.stat_count.ptr, 8), "psh_memcpy_d2h")
    if conditional and int(wet[0]) < 2:
        return _to_reference("fewer than two wet pixels to condition on", R, ref_args, ref_kwargs)
    mu, sigma = (float(v) for v in _host_pairs(masked_moments(clean, chain.stat_mask, chain.stat_count), 1)[0])
    if not (np.isfinite(mu) and np.isfinite(sigma) and sigma > 0.0):
        return _to_reference("the conditioned sample is degenerate (sigma = %r)" % sigma, R, ref_args, ref_kwargs)
    _lib.check(lib.psh_noise_adj_centre_dev(clean.ptr, plane, mu), "psh_noise_adj_centre_dev")
    stds_R = chain.level_stats(clean, 1)[0, :, 1]

    # utils.py:103-106 on the host, the streams themselves on the device
    randstates = _seed_chain(seed, int(num_iter))
    num_iter = len(randstates)
    drs = DeviceRandomStates(randstates, plane, n_draws=1)
    try:
        white = drs.randn(m, n)
        d_filter = _device_weights(noise_filter["field"])
        budget = BATCH_BYTES if _batch_bytes is None else int(_batch_bytes)
        per_batch = int(max(1, min(num_iter, budget // _per_realisation_bytes(m, n, L, spectral))))
        stds_N = np.empty((num_iter, L), dtype=np.float64)
        for first in range(0, num_iter, per_batch):
            nb = min(per_batch, num_iter - first)
            fields = DeviceArray((nb, m, n), np.float64)
            for j in range(nb):  # fftgenerators.py:420-433
                _lib.check(lib.psh_noise_filter_dev(white.view(first + j).ptr, d_filter.ptr, m, n, fields.view(j).ptr),
                           "psh_noise_filter_dev")
            prepare(fields, chain.mask, sigma, mu, R_thr_2)  # utils.py:113-118
            stds_N[first:first + nb] = chain.level_stats(fields, nb)[:, :, 1]  # utils.py:119-121
        if _randstates_out is not None:
            drs.sync_back()
            _randstates_out.extend(randstates)
        else:
            drs.check()
    finally:
        drs.close()
    # utils.py:135
    return stds_R / np.mean(stds_N, axis=0)
