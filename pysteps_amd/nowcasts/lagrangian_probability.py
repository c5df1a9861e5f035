"""The local Lagrangian probability nowcast on the GPU (mirror of pysteps/nowcasts/lagrangian_probability.py
``forecast``, Germann and Zawadzki 2004), registered as ``"lagrangian_probability_hip"``.

The probability of exceeding ``threshold`` is the fraction of the valid pixels of a neighbourhood of the advected
field that exceed it; the neighbourhood (a disc, a square below diameter 5) grows with the lead time,
``scale = int(timestep * slope)``.  Both stages run on the device and the advected stack never leaves HBM:

* the advection: :func:`pysteps_amd.nowcasts.extrapolation.forecast` on resident arrays (the HIP semi-Lagrangian
  extrapolator);
* the neighbourhood fraction: ``psh_lagprob_dev`` (csrc/lagprob.hip).  The reference convolves two 0/1 maps with a
  0/1 kernel, through SciPy's FFT path for every scale >= 3, and so returns quotients of small integers with an
  error near 1e-7.  The kernels count instead: row prefix counts of both maps, then per pixel one difference per
  kernel row over the spans of :func:`kernel_spans`.  The result is the correctly rounded quotient, deterministic.

NumPy inputs give a NumPy array, DeviceArray inputs a resident float64 DeviceArray.  What the device path does not
take (another extrapolation method, a scale above 255, a width above 65535, an ``interp_order`` the extrapolator
hands to the reference) goes to the reference with a warning when pysteps is importable and raises
``NotImplementedError`` otherwise.
"""

import warnings

import numpy as np

from .. import _lib
from .._reference import lookup
from ..device import DeviceArray
from . import extrapolation

__all__ = ["forecast", "kernel_spans", "probability_stage", "MAX_SCALE", "MAX_WIDTH"]

MAX_SCALE = 255  # csrc/lagprob.hip kLagMaxScale
MAX_WIDTH = 65535  # csrc/lagprob.hip kLagMaxWidth
_EXTRAPOLATORS = ("semilagrangian", "semilagrangian_hip")
# device time of the last call (ms): {"extrapolation", "probability"}, from events on the library stream
# (tools/lagprob_quick.py)
last_run_stats = {}


def _kernel_support(scale):
    """First and last column of every row of the reference's ``_get_kernel(scale)``: all of the row below scale 5,
    else the disc ``(i - mid)**2 + (j - mid)**2 <= mid**2`` with ``mid = scale // 2`` on the scale x scale grid."""
    if scale < 5:
        return np.zeros(scale, dtype=np.int64), np.full(scale, scale - 1, dtype=np.int64)
    mid = scale // 2
    ii, jj = np.mgrid[:scale, :scale]
    disc = (ii - mid) ** 2 + (jj - mid) ** 2 <= mid**2
    jlo = disc.argmax(axis=1)
    jhi = scale - 1 - disc[:, ::-1].argmax(axis=1)
    # every row of the grid meets the disc (|i - mid| <= mid) in one run of columns
    assert np.array_equal(disc.sum(axis=1), jhi - jlo + 1)
    return jlo, jhi


def kernel_spans(scale):
    """The kernel of ``scale`` as ``scipy.signal.convolve(..., mode="same")`` applies it, row by row:
    ``(dy, lo, hi)``, int32 arrays of ``scale`` entries.  Output pixel ``(y, x)`` sums the input pixels
    ``(y + dy[t], x + lo[t] .. x + hi[t])``.  ``convolve`` flips the kernel and ``mode="same"`` takes
    ``full[y + c, x + c]`` with ``c = (scale - 1) // 2``, so kernel entry ``(i, j)`` meets input pixel
    ``(y + c - i, x + c - j)``; the disc is not symmetric for even scales, so the flip matters."""
    scale = int(scale)
    if scale < 1:
        raise ValueError("kernel_spans: scale %d" % scale)
    c = (scale - 1) // 2
    jlo, jhi = _kernel_support(scale)
    i = scale - 1 - np.arange(scale)  # t = 0 is the topmost input row: dy = c - i = t + c - scale + 1
    return (c - i).astype(np.int32), (c - jhi[i]).astype(np.int32), (c - jlo[i]).astype(np.int32)


def _scales(leads, slope):
    return [int(t * slope) for t in leads]


def probability_stage(fields, threshold, scales):
    """The neighbourhood fractions of an advected stack: ``fields`` a (T, m, n) float32 or float64 DeviceArray,
    ``scales`` one kernel size per plane (0 .. 255; 0 gives the 0/1 exceedance map, which is what the 1 x 1 kernel
    gives).  Returns a float64 DeviceArray (T, m, n), NaN where ``fields`` is NaN."""
    if fields.ndim != 3 or fields.dtype not in (np.float32, np.float64):
        raise ValueError("probability_stage: a (T, m, n) float32 or float64 DeviceArray expected")
    T, m, n = fields.shape
    sc = np.ascontiguousarray([max(int(s), 1) for s in scales], dtype=np.int32)
    if sc.size != T:
        raise ValueError("probability_stage: %d scales for %d planes" % (sc.size, T))
    if sc.max() > MAX_SCALE or n > MAX_WIDTH:
        raise NotImplementedError("probability_stage: scale %d, width %d (at most %d, %d)" % (sc.max(), n, MAX_SCALE, MAX_WIDTH))
    spans = {s: kernel_spans(s) for s in set(sc.tolist())}
    lo = np.ascontiguousarray(np.concatenate([spans[s][1] for s in sc.tolist()]), dtype=np.int32)
    hi = np.ascontiguousarray(np.concatenate([spans[s][2] for s in sc.tolist()]), dtype=np.int32)
    out = DeviceArray((T, m, n), np.float64)
    _lib.check(_lib.lib().psh_lagprob_dev(fields.ptr, int(fields.dtype == np.float64), T, m, n, float(threshold),
                                          sc.ctypes.data, lo.ctypes.data, hi.ctypes.data, out.ptr), "psh_lagprob_dev")
    return out


def _unsupported(precip, leads, slope, extrap_method, extrap_kwargs):
    if not isinstance(extrap_method, str) or extrap_method.lower() not in _EXTRAPOLATORS:
        return "extrap_method=%r" % (extrap_method,)
    kw = extrap_kwargs or {}
    if kw.get("interp_order", 1) not in (0, 1, 2, 3, 4, 5):
        return "interp_order=%r" % (kw.get("interp_order"),)
    if kw.get("return_displacement", False):
        return "return_displacement in extrap_kwargs"
    try:
        scales = _scales(leads, slope)
    except Exception:  # whatever the reference makes of such lead times or such a slope
        return "timesteps=%r with slope=%r" % (leads, slope)
    if any(s < 0 or s > MAX_SCALE for s in scales):
        return "scale %d (the device path takes 0 .. %d)" % (max(scales, key=abs), MAX_SCALE)
    if precip.shape[1] > MAX_WIDTH:
        return "width %d (above %d)" % (precip.shape[1], MAX_WIDTH)
    return None


def _to_device_f32(a):
    if isinstance(a, DeviceArray):
        if a.dtype == np.float32:
            return a
        if a.dtype != np.float64:
            raise ValueError("device-resident precip/velocity must be float32 or float64")
        out = DeviceArray(a.shape, np.float32)
        _lib.check(_lib.lib().psh_convert_dev(a.ptr, out.ptr, a.size, 0), "psh_convert_dev")
        return out
    a = np.asarray(np.ma.getdata(a) if np.ma.isMaskedArray(a) else a)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return DeviceArray.from_host(a, dtype=np.float32)


def _check_host_values(precip, velocity):
    """The value checks the reference's extrapolator makes on its NumPy inputs (semilagrangian.py:112-123), with its
    messages; resident inputs are taken as they are, like the extrapolator takes them."""
    allow = bool(np.any(~np.isfinite(precip)))  # nowcasts/extrapolation.py:76
    if not allow and np.any(~np.isfinite(velocity)):
        raise ValueError("velocity contains non-finite values")
    if np.all(~np.isfinite(precip)):
        raise ValueError("precip contains only non-finite values")
    if np.all(~np.isfinite(velocity)):
        raise ValueError("velocity contains only non-finite values")


def forecast(precip, velocity, timesteps, threshold, extrap_method="semilagrangian", extrap_kwargs=None, slope=5):
    """Generate a probability nowcast by a local Lagrangian approach: the probability of exceeding ``threshold``,
    P(precip >= threshold) (reference: pysteps/nowcasts/lagrangian_probability.py; parameters and return value as
    documented there): a float64 array ``(num_timesteps, m, n)``, NaN where the advected field is NaN.  DeviceArray
    inputs give a DeviceArray output."""
    if isinstance(timesteps, int) and timesteps > 0:
        leads = np.arange(1, timesteps + 1)
    elif not isinstance(timesteps, list):
        raise ValueError(f"invalid value for argument 'timesteps': {timesteps}")
    else:
        leads = timesteps
    extrapolation._check_inputs(precip, velocity, leads)
    resident_in = isinstance(precip, DeviceArray)
    if resident_in != isinstance(velocity, DeviceArray):
        raise ValueError("precip and velocity must both be NumPy arrays or both be DeviceArrays")

    why = _unsupported(precip, leads, slope, extrap_method, extrap_kwargs)
    if why is not None:
        ref = lookup("nowcasts.lagrangian_probability", "forecast", forecast)
        if ref is None or resident_in:
            raise NotImplementedError("pysteps_amd lagrangian_probability: %s is not implemented on the device and "
                                      "pysteps is not importable for the reference's forecast" % why)
        warnings.warn("pysteps_amd lagrangian_probability: %s - running the reference's forecast" % why, stacklevel=2)
        return ref(precip, velocity, timesteps, threshold, extrap_method=extrap_method, extrap_kwargs=extrap_kwargs,
                   slope=slope)

    if not resident_in:
        _check_host_values(np.asarray(precip), np.asarray(velocity))
    kw = dict() if extrap_kwargs is None else dict(extrap_kwargs)
    if kw.get("displacement_prev") is not None and not isinstance(kw["displacement_prev"], DeviceArray):
        kw["displacement_prev"] = DeviceArray.from_host(np.ascontiguousarray(kw["displacement_prev"], dtype=np.float64))

    from ..device import Event  # noqa: PLC0415

    ev0 = Event().record()
    advected = extrapolation.forecast(_to_device_f32(precip), _to_device_f32(velocity), leads, extrap_method, kw)
    ev1 = Event().record()
    out = probability_stage(advected, threshold, _scales(leads, slope))
    ev2 = Event().record()
    del advected
    result = out if resident_in else out.to_host()
    _lib.check(_lib.lib().psh_sync(), "psh_sync")
    last_run_stats.clear()
    last_run_stats.update(extrapolation=ev0.elapsed_ms(ev1), probability=ev1.elapsed_ms(ev2))
    return result
