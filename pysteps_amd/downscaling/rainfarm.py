"""RainFARM stochastic downscaling on the GPU (mirror of pysteps/downscaling/rainfarm.py ``downscale``), registered
as ``"rainfarm_hip"``.

The reference fills a coarse rain field with small-scale variability from a power-law Gaussian random field
(Rebora et al. 2006): ``Re(ifft2(exp(2 pi i U) sqrt(f^-alpha)))`` with uniforms ``U`` on the fine grid, standardised,
exponentiated, and scaled so that its block means follow the coarse field.  Here (csrc/rainfarm.hip):

* the uniforms: NumPy's MT19937 stream continued on the device (``DeviceRandomStates.uniform``) and written back, so
  the generator - the global one, or ``randstate`` - is left where the reference's ``np.random.rand(M, N)`` leaves it
  (a ``DeviceRandomStates`` handle the caller keeps is drawn from as it is, without the hand-over);
* the spectrum: its Hermitian part straight into ``rfft2`` layout (``psh_rainfarm_spectrum_dev``), then the existing
  ``irfft2`` - half the transform and half the plane of the reference's complex ``ifft2``;
* ``noise.std()``: mean, then mean squared deviation, double-double sums in a fixed order (``psh_rainfarm_std_dev``);
* ``exp(noise / std)`` and its ``ds x ds`` block means in one pass (``psh_rainfarm_exp_dev``);
* the finish in one pass (``psh_rainfarm_finish_dev``): with a smoothing kernel the reference convolves two expanded
  planes (and the all-ones mask) with a ``(2 r + 1)^2`` kernel; both planes are constant on coarse cells, so a
  pixel's average is a sum over at most ``(2 + 2 r // ds)^2`` cells of kernel-weight partial sums that depend on the
  pixel's phase inside its cell alone (:func:`weight_table`, built on the host once per kernel and factor).

``alpha=None``: ``rfft2`` of the low-resolution field on the device, the half spectrum downloaded and mirrored, then
the reference's ``_log_slope`` arithmetic (``np.polyfit``) on the host.  The estimate always runs in float64 on the
widened field: for float64 fields it is the reference's estimate up to the transform's rounding; for float32 NumPy
fields the reference (numpy >= 2) estimates from a complex64 transform and differs at that level.

A NumPy field gives a float64 NumPy array, a DeviceArray gives a DeviceArray (float32 for a float32 field, rounded once
at the final store).  ``spectral_fusion=True``, shapes the device FFT does not take and dtypes other than float32 /
float64 go to the reference with a ``RuntimeWarning`` when pysteps is importable and raise ``NotImplementedError``
otherwise.  :func:`downscale_table` makes K realisations in one batch.
"""

import warnings

import numpy as np

from .. import _lib
from .._reference import lookup
from ..device import DeviceArray, Event, synchronize
from ..noise.randstate import DeviceRandomStates
from ..utils import fft as hip_fft

__all__ = ["downscale", "downscale_table", "noise_field", "finish", "estimate_alpha", "kernel_radius", "make_kernel",
           "weight_table"]

KERNEL_TYPES = ["gaussian", "tophat", "uniform"]  # the reference's _make_kernel, in its order
# device time of the last call (ms): {"draw", "synthesis", "transform", "reduce_exp", "finish", "total"}
last_run_stats = {}
CHUNKED_DRAW = 1 << 20  # uniforms per call from which the draw is produced in chunks
_marks = []
_tables = {}


def _mark(name):
    _marks.append((name, Event().record()))


def kernel_radius(ds_factor):
    """The reference's ``_compute_kernel_radius``."""
    return int(round(ds_factor / np.sqrt(np.pi)))


def make_kernel(kernel_type, ds_factor):
    """The reference's normalised smoothing kernel, (2 r + 1, 2 r + 1) float64."""
    radius = kernel_radius(ds_factor)
    if kernel_type == "gaussian":
        sigma = ds_factor / 2
        sigma2 = sigma * sigma
        x = np.arange(-radius, radius + 1)
        kern1d = np.exp(-0.5 / sigma2 * x**2)
        kern2d = np.outer(kern1d, kern1d)
        return kern2d / kern2d.sum()
    mx, my = np.mgrid[-radius : radius + 0.01, -radius : radius + 0.01]
    tophat = ((mx**2 + my**2) <= radius**2).astype(float)
    return tophat / tophat.sum()


def weight_table(kernel, ds_factor):
    """``(table, amin)``: ``table[py, px, a, b]`` is the sum of the kernel's taps that reach the coarse cell
    ``(I + a + amin, J + b + amin)`` from a fine pixel at phase ``(py, px)`` of cell ``(I, J)``."""
    ds = int(ds_factor)
    r = (kernel.shape[0] - 1) // 2
    amin = -((r + ds - 1) // ds)
    na = (ds - 1 + r) // ds - amin + 1
    cell = (np.arange(ds)[:, None] + np.arange(-r, r + 1)[None, :]) // ds - amin  # (phase, tap) -> cell slot
    hot = (cell[:, None, :] == np.arange(na)[None, :, None]).astype(np.float64)  # (phase, slot, tap)
    rows = hot @ np.asarray(kernel, dtype=np.float64)  # (py, a, tap_x)
    table = np.einsum("pau,qbu->pqab", rows, hot)
    return np.ascontiguousarray(table), amin


def _log_slope(log_k, log_power_spectrum):
    """The reference's ``_log_slope``."""
    lk_min = log_k.min()
    lk_max = log_k.max()
    lk_range = lk_max - lk_min
    lk_min += (1 / 6) * lk_range
    lk_max -= (1 / 6) * lk_range
    selected = (lk_min <= log_k) & (log_k <= lk_max)
    lk_sel = log_k[selected]
    ps_sel = log_power_spectrum[selected]
    alpha = np.polyfit(lk_sel, ps_sel, 1)[0]
    alpha = -alpha
    return alpha


def _freq_array(shape, ds_factor=1):
    freq_i = np.fft.fftfreq(shape[0] * ds_factor, d=1 / ds_factor)
    freq_j = np.fft.fftfreq(shape[1] * ds_factor, d=1 / ds_factor)
    return np.sqrt(freq_i[:, None] ** 2 + freq_j[None, :] ** 2)


def estimate_alpha(field):
    """The reference's ``_estimate_alpha`` of an (m, n) float64 field (DeviceArray or NumPy): the transform on the
    device, ``log |F|^2`` of the mirrored half spectrum and the fit on the host."""
    m, n = (int(s) for s in field.shape)
    half = hip_fft.rfft2(field)
    if isinstance(half, DeviceArray):
        half = half.to_host()
    nc = n // 2 + 1
    log_half = np.log(np.abs(half) ** 2)
    log_power_spectrum = np.empty((m, n), dtype=np.float64)
    log_power_spectrum[:, :nc] = log_half
    if n > nc:  # F[k, l] = conj(F[-k, -l])
        log_power_spectrum[:, nc:] = log_half[(-np.arange(m)) % m][:, n - np.arange(nc, n)]
    k = _freq_array((m, n))
    valid = (k != 0) & np.isfinite(log_power_spectrum)
    return _log_slope(np.log(k[valid]), log_power_spectrum[valid])


def _as_stack(x, dtype, what):
    """(K, rows, cols) DeviceArray of ``dtype`` and whether a leading axis was added."""
    if not isinstance(x, DeviceArray):
        x = DeviceArray.from_host(np.ascontiguousarray(x, dtype=dtype))
    if x.dtype != np.dtype(dtype) or x.ndim not in (2, 3):
        raise ValueError("%s must be a 2-d or 3-d %s array" % (what, np.dtype(dtype)))
    if x.ndim == 2:
        return DeviceArray((1,) + x.shape, x.dtype, ptr=x.ptr, owner=x), True
    return x, False


def noise_field(u, alpha, lowres_shape, ds_factor):
    """The reference's ``_compute_noise_field`` with the uniforms given: ``u`` (M, N) or (K, M, N) float64 ->
    the correlated real field of the same shape, a float64 DeviceArray.  ``alpha``: one slope or K."""
    u, single = _as_stack(u, np.float64, "u")
    K, M, N = u.shape
    ds = int(ds_factor)
    if (M, N) != (int(lowres_shape[0]) * ds, int(lowres_shape[1]) * ds):
        raise ValueError("u has shape %s, expected %s" % ((M, N), (int(lowres_shape[0]) * ds, int(lowres_shape[1]) * ds)))
    alphas = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (K,)))
    d_alphas = DeviceArray.from_host(alphas)
    nc = N // 2 + 1
    half = DeviceArray((K, M, nc), np.complex128)
    noise = DeviceArray((K, M, N), np.float64)
    lib = _lib.lib()
    # np.fft.fftfreq(M, d=1 / ds): integer bins times 1.0 / (M * d)
    vi, vj = 1.0 / (M * (1 / ds)), 1.0 / (N * (1 / ds))
    _mark("synthesis")
    _lib.check(lib.psh_rainfarm_spectrum_dev(u.ptr, d_alphas.ptr, K, M, N, vi, vj, half.ptr), "psh_rainfarm_spectrum_dev")
    _mark("transform")
    for p in range(K):
        _lib.check(lib.psh_fft_irfft2_dev(half.ptr + p * M * nc * 16, M, N, noise.ptr + p * M * N * 8), "psh_fft_irfft2_dev")
    _mark("transform_end")
    return noise.view(0) if single else noise


def _table_for(kernel_type, ds):
    key = (kernel_type, ds)
    if key not in _tables:
        _tables.clear()  # one at a time: a table has 9 ds^2 entries or more
        _tables[key] = weight_table(make_kernel(kernel_type, ds), ds)
    return _tables[key]


def finish(precip, noise, ds_factor, kernel_type=None, threshold=None, out_dtype=np.float64, _in_place=False):
    """Everything after the transform: ``precip`` (m, n) or (K, m, n) float64, ``noise`` (M, N) or (K, M, N) float64
    -> the downscaled field(s), a DeviceArray of ``out_dtype`` (float64 or float32) shaped like ``noise``.  One
    low-resolution plane serves every realisation."""
    if kernel_type and kernel_type not in KERNEL_TYPES:
        raise ValueError(f"kernel type '{kernel_type}' is invalid, available kernels: {KERNEL_TYPES}")
    out_dtype = np.dtype(out_dtype)
    if out_dtype not in (np.float32, np.float64):
        raise ValueError("out_dtype must be float32 or float64")
    noise, single = _as_stack(noise, np.float64, "noise")
    precip, _ = _as_stack(precip, np.float64, "precip")
    K, M, N = noise.shape
    Kp, m, n = precip.shape
    ds = int(ds_factor)
    if (M, N) != (m * ds, n * ds) or Kp not in (1, K):
        raise ValueError("noise %s does not match precip %s at ds_factor=%d" % (noise.shape, precip.shape, ds))
    lib = _lib.lib()
    stats = DeviceArray((K, 2), np.float64)
    agg = DeviceArray((K, m, n), np.float64)
    e = noise if _in_place else DeviceArray((K, M, N), np.float64)
    _mark("reduce_exp")
    _lib.check(lib.psh_rainfarm_std_dev(noise.ptr, K, M * N, stats.ptr), "psh_rainfarm_std_dev")
    _lib.check(lib.psh_rainfarm_exp_dev(noise.ptr, stats.ptr, K, m, n, ds, e.ptr, agg.ptr), "psh_rainfarm_exp_dev")
    _mark("finish")
    table, na, amin = None, 0, 0
    if kernel_type:
        host_table, amin = _table_for(kernel_type, ds)
        na = int(host_table.shape[2])
        table = DeviceArray.from_host(host_table)
    out = DeviceArray((K, M, N), out_dtype)
    _lib.check(lib.psh_rainfarm_finish_dev(e.ptr, precip.ptr, Kp, agg.ptr, K, m, n, ds, table.ptr if table is not None else None,
                                           na, amin, int(threshold is not None), float(threshold) if threshold is not None else 0.0,
                                           int(out_dtype == np.float32), out.ptr), "psh_rainfarm_finish_dev")
    _mark("finish_end")
    return out.view(0) if single else out


def _unsupported(shape, dtype, ds, spectral_fusion):
    """Why the device path does not take this call (None if it does)."""
    if spectral_fusion:
        return "spectral_fusion=True (the reference's own result is uncertain at the 1e-8 level there, DESIGN.md 3.15)"
    if len(shape) != 2:
        return "a %d-dimensional field" % len(shape)
    if np.dtype(dtype) not in (np.float32, np.float64):
        return "dtype %s (the device path takes float32 and float64)" % np.dtype(dtype)
    hi = (shape[0] * ds, shape[1] * ds)
    if not hip_fft.supported_shape(hi):
        return "high-resolution shape %s (not taken by the device FFT)" % (hi,)
    return None


def _run_reference(why, fields, resident, ds_factor, randstate, kw):
    """The reference's ``downscale`` on every field in turn, drawing from ``randstate`` when one is given."""
    ref = lookup("downscaling.rainfarm", "downscale", downscale)
    if ref is None:
        raise NotImplementedError("pysteps_amd rainfarm: %s, and pysteps is not importable for the reference's downscale" % why)
    if isinstance(randstate, DeviceRandomStates):
        raise ValueError("pysteps_amd rainfarm: %s, and a DeviceRandomStates cannot feed the reference's downscale" % why)
    warnings.warn("pysteps_amd rainfarm: %s - running the reference's downscale" % why, RuntimeWarning, stacklevel=3)
    saved = None
    if randstate is not None:
        saved = np.random.get_state()
        np.random.set_state(randstate.get_state())
    try:
        return [ref(f.to_host() if resident else f, ds_factor, **kw) for f in fields]
    finally:
        if saved is not None:
            randstate.set_state(np.random.get_state())
            np.random.set_state(saved)


def _nonfinite(x):
    import ctypes  # noqa: PLC0415

    flag = ctypes.c_int(0)
    _lib.check(_lib.lib().psh_darts_nonfinite_dev(x.ptr, int(x.dtype == np.float32), x.size, ctypes.byref(flag)),
               "psh_darts_nonfinite_dev")
    return bool(flag.value)


def _downscale(precip, ds_factor, K, stacked, alpha, threshold, return_alpha, kernel_type, spectral_fusion, randstate):
    resident = isinstance(precip, DeviceArray)
    if not resident:
        precip = np.asarray(precip)
    # the reference's checks, texts and order
    if not resident and not np.isfinite(precip).all():
        raise ValueError("All values in 'precip' must be finite.")
    if resident and precip.dtype in (np.float32, np.float64) and _nonfinite(precip):
        raise ValueError("All values in 'precip' must be finite.")
    if not isinstance(ds_factor, int) or ds_factor <= 0:
        raise ValueError("'ds_factor' must be a positive integer.")
    if kernel_type and kernel_type not in KERNEL_TYPES:
        raise ValueError(f"kernel type '{kernel_type}' is invalid, available kernels: {KERNEL_TYPES}")

    shape = tuple(int(s) for s in precip.shape)
    why = _unsupported(shape[1:] if stacked else shape, precip.dtype, ds_factor, spectral_fusion)
    if why is not None:
        kw = dict(alpha=alpha, threshold=threshold, return_alpha=return_alpha, kernel_type=kernel_type,
                  spectral_fusion=spectral_fusion)
        fields = [precip.view(j) if resident else precip[j] for j in range(K)] if stacked else [precip] * K
        res = _run_reference(why, fields, resident, ds_factor, randstate, kw)
        fields_out = np.stack([r[0] if return_alpha else r for r in res])
        alphas = np.array([r[1] for r in res]) if return_alpha else None
        return (DeviceArray.from_host(fields_out) if resident else fields_out), alphas

    out_dtype = np.float32 if resident and precip.dtype == np.float32 else np.float64
    if resident and precip.dtype == np.float32:
        wide = DeviceArray(shape, np.float64)
        _lib.check(_lib.lib().psh_convert_dev(precip.ptr, wide.ptr, precip.size, 1), "psh_convert_dev")
        precip = wide
    elif not resident:
        precip = DeviceArray.from_host(np.ascontiguousarray(precip, dtype=np.float64))
    m, n = shape[-2:]
    M, N = m * ds_factor, n * ds_factor

    if alpha is None:
        planes = [precip.view(j) for j in range(K)] if stacked else [precip]
        alphas = np.array([estimate_alpha(p) for p in planes], dtype=np.float64)
        alphas = np.ascontiguousarray(np.broadcast_to(alphas, (K,)))
    else:
        alphas = np.full(K, alpha, dtype=np.float64)

    _marks.clear()
    _mark("draw")
    if isinstance(randstate, DeviceRandomStates):
        # the caller's handle: no hand-over, no write-back (its sync_back() does that when the caller wants it)
        if randstate.n != 1 or randstate.max_draw < K * M * N:
            raise ValueError("randstate: a DeviceRandomStates of one generator with max_draw >= %d is needed" % (K * M * N))
        u = randstate.uniform(0.0, 1.0, K, M, N)
    else:
        # a long draw is cut into chunks that start from MT19937 jump-ahead states (hundreds of workgroups instead of
        # one); building those states costs more than a short draw takes
        gen = DeviceRandomStates([np.random.mtrand._rand if randstate is None else randstate], K * M * N,
                                 n_draws=1 if K * M * N >= CHUNKED_DRAW else None)
        try:
            u = gen.uniform(0.0, 1.0, K, M, N)
            gen.sync_back()
        finally:
            gen.close()
    noise = noise_field(u.view(0), alphas, (m, n), ds_factor)
    del u
    out = finish(precip, noise, ds_factor, kernel_type, threshold, out_dtype, _in_place=True)
    synchronize()
    marks = dict(_marks)
    last_run_stats.clear()
    last_run_stats.update(draw=marks["draw"].elapsed_ms(marks["synthesis"]),
                          synthesis=marks["synthesis"].elapsed_ms(marks["transform"]),
                          transform=marks["transform"].elapsed_ms(marks["transform_end"]),
                          reduce_exp=marks["reduce_exp"].elapsed_ms(marks["finish"]),
                          finish=marks["finish"].elapsed_ms(marks["finish_end"]),
                          total=marks["draw"].elapsed_ms(marks["finish_end"]))
    _marks.clear()
    return (out if resident else out.to_host()), alphas


def downscale(precip, ds_factor, alpha=None, threshold=None, return_alpha=False, kernel_type=None, spectral_fusion=False,
              randstate=None):
    """Downscale a rainfall field by increasing its spatial resolution by a positive integer factor (reference:
    pysteps/downscaling/rainfarm.py ``downscale``; arguments, checks and return value as documented there).

    ``precip``: (m, n) NumPy array or DeviceArray.  ``randstate``: a ``numpy.random.RandomState`` to draw from
    instead of NumPy's global generator, or a :class:`~pysteps_amd.noise.randstate.DeviceRandomStates` of one
    generator that the caller keeps across calls (the hand-over of a host generator - ring, jump-ahead start states,
    write-back, release - costs several times the rest of a 4096^2 call; the caller's ``sync_back()`` writes the state
    back when it is wanted).  Returns the (m ds_factor, n ds_factor) field - float64 NumPy for a NumPy
    field, a DeviceArray for a DeviceArray (float32 for a float32 one) - and ``alpha`` with ``return_alpha=True``.
    For a float32 NumPy field with ``alpha=None`` the reference (numpy >= 2) estimates the slope from a complex64
    transform; here the field is widened first."""
    out, alphas = _downscale(precip, ds_factor, 1, False, alpha, threshold, return_alpha, kernel_type, spectral_fusion,
                             randstate)
    field = out.view(0) if isinstance(out, DeviceArray) else out[0]
    if return_alpha:
        return field, (alpha if alpha is not None else alphas[0])
    return field


def downscale_table(precip, ds_factor, n_realizations=None, **kwargs):
    """K realisations in one batch: a (K, m, n) stack gives one realisation per plane, in order; a single (m, n)
    field with ``n_realizations=K`` gives K realisations of it.  The (K, M, N) result holds the values K successive
    :func:`downscale` calls give and leaves the generator where they leave it; keywords as for :func:`downscale`
    (``return_alpha=True`` adds the K slopes as an array)."""
    ndim = precip.ndim if isinstance(precip, DeviceArray) else np.ndim(precip)
    if ndim == 3:
        K = int(precip.shape[0] if isinstance(precip, DeviceArray) else np.shape(precip)[0])
        if n_realizations is not None and int(n_realizations) != K:
            raise ValueError("n_realizations=%d does not match the %d planes of the stack" % (n_realizations, K))
        stacked = True
    elif ndim == 2:
        if n_realizations is None or int(n_realizations) < 1:
            raise ValueError("n_realizations must be a positive integer for a single field")
        K, stacked = int(n_realizations), False
    else:
        raise ValueError("precip must be an (m, n) field or a (K, m, n) stack")
    kw = dict(alpha=None, threshold=None, return_alpha=False, kernel_type=None, spectral_fusion=False, randstate=None)
    unknown = set(kwargs) - set(kw)
    if unknown:
        raise TypeError("downscale_table() got an unexpected keyword argument %r" % sorted(unknown)[0])
    kw.update(kwargs)
    out, alphas = _downscale(precip, ds_factor, K, stacked, kw["alpha"], kw["threshold"], kw["return_alpha"],
                             kw["kernel_type"], kw["spectral_fusion"], kw["randstate"])
    return (out, alphas) if kw["return_alpha"] else out
