"""The Proesmans motion estimate on the GPU (mirror of pysteps/motion/proesmans.py ``proesmans`` and its Cython module
``_proesmans.pyx``; Proesmans et al. 1994), registered as ``"proesmans_hip"``.

The method relaxes a forward and a backward flow field against each other on an image pyramid: per level and iteration
it recomputes the two consistency maps and then updates every interior pixel of both fields IN PLACE in raster order
- a Gauss-Seidel sweep: a pixel reads its three upper neighbours and its left neighbour after the sweep wrote them and
the other four before.  That order is part of the algorithm (a sweep from the old field alone moves the result by
pixels), and the device keeps it: in t = x + 2 y every pixel depends on smaller t only, so a wave takes 64 rows, one
lane per row, and walks along t; tiles of that walk run one anti-diagonal per launch (csrc/proesmans.hip).

All arithmetic is float64 with the reference's operations in the reference's order and without fused multiply-adds, so
every stage equals the reference's bit for bit - but for the sum ``c_sum`` behind ``K = 0.9 c_sum / c_count`` of the
consistency maps: the reference adds in raster order, the device forms a double-double sum in a fixed order and rounds
once.  The whole result therefore equals the reference evaluated with an exactly rounded ``c_sum``.

NumPy in gives float64 NumPy out.  A DeviceArray (2, m, n) in gives DeviceArrays out, float32 for float32 frames (rounded
once at the final store; the form ``semilagrangian_hip`` takes).  float32 host arrays are widened - the reference itself
rejects them at its typed memoryview.  ``filter_std > 0`` runs SciPy's ``gaussian_filter`` on the host on the scaled
frames: one round trip of two frames.  Non-finite input, or a coarsest pyramid level with a side below 3, goes to the
reference with a RuntimeWarning when pysteps is importable and raises ``NotImplementedError`` otherwise.
"""

import ctypes
import warnings

import numpy as np

from .. import _lib
from .._reference import lookup
from ..device import DeviceArray, Event, synchronize

__all__ = ["proesmans", "scale_frames", "pyramid_level", "gradients", "consistency_maps", "sweep", "next_level",
           "advection_field", "launches_per_iteration"]

# device time of the last call (ms): {"scale", "filter", "flow", "total"} and the launches of one iteration at level 0
last_run_stats = {}


def _check_input_frames(input_images):
    """``pysteps.decorators.check_input_frames(2, 2)``"""
    if input_images.ndim != 3:
        raise ValueError(
            "input_images dimension mismatch.\n"
            f"input_images.shape: {str(input_images.shape)}\n"
            "(t, x, y ) dimensions expected"
        )
    num_of_frames = input_images.shape[0]
    if 2 < num_of_frames > 2:
        raise ValueError(
            f"input_images frames {num_of_frames} mismatch.\n"
            "Minimum frames: 2\n"
            "Maximum frames: 2\n"
        )
    if num_of_frames < 2:
        raise IndexError("index -2 is out of bounds for axis 0 with size %d" % num_of_frames)


def _f64(x, shape):
    if not isinstance(x, DeviceArray) or x.dtype != np.float64 or tuple(x.shape) != tuple(shape):
        raise ValueError("expected a float64 DeviceArray of shape %s" % (tuple(shape),))
    return x


def scale_frames(frames):
    """``(im - min) / (max - min) * 255.0`` over both frames (left alone when max - min <= 1e-8).  ``frames``: float32 or
    float64 DeviceArray; returns (float64 DeviceArray, (min, max, number of non-finite values))."""
    if frames.dtype not in (np.float32, np.float64):
        raise ValueError("device-resident frames must be float32 or float64 (got %s)" % frames.dtype)
    out = DeviceArray(frames.shape, np.float64)
    rng = (ctypes.c_double * 3)()
    _lib.check(_lib.lib().psh_proesmans_scale_dev(frames.ptr, int(frames.dtype == np.float32), frames.size, out.ptr, rng),
               "psh_proesmans_scale_dev")
    return out, (rng[0], rng[1], int(rng[2]))


def pyramid_level(src):
    """The next pyramid level of a (m, n) float64 DeviceArray: (int(m/2), int(n/2))."""
    m, n = src.shape
    _f64(src, (m, n))
    out = DeviceArray((m // 2, n // 2), np.float64)
    _lib.check(_lib.lib().psh_proesmans_pyramid_dev(src.ptr, m, n, out.ptr), "psh_proesmans_pyramid_dev")
    return out


def gradients(frame):
    """``_compute_gradients``: (2, m, n) from a (m, n) float64 DeviceArray."""
    m, n = frame.shape
    _f64(frame, (m, n))
    out = DeviceArray((2, m, n), np.float64)
    _lib.check(_lib.lib().psh_proesmans_gradients_dev(frame.ptr, m, n, out.ptr), "psh_proesmans_gradients_dev")
    return out


def consistency_maps(V, stages=False):
    """``_compute_consistency_maps`` of V (2, 2, m, n): GAMMA (2, m, n).  ``stages=True`` returns (GAMMA, raw c planes,
    stats) with stats (2, 4) = per direction {c_sum, c_count, K, 0}."""
    m, n = V.shape[2:]
    _f64(V, (2, 2, m, n))
    gamma = DeviceArray((2, m, n), np.float64)
    raw = DeviceArray((2, m, n), np.float64) if stages else None
    stats = DeviceArray((2, 4), np.float64) if stages else None
    _lib.check(_lib.lib().psh_proesmans_consistency_dev(V.ptr, m, n, gamma.ptr, raw.ptr if stages else None,
                                                        stats.ptr if stages else None), "psh_proesmans_consistency_dev")
    return (gamma, raw, stats) if stages else gamma


def sweep(V, gamma, frames, grads, lam):
    """One iteration's update of V (2, 2, m, n) in place, both directions, in the reference's order, then the edge
    fill.  ``frames`` (2, m, n), ``grads`` (2, 2, m, n) = [frame][gx, gy], ``gamma`` (2, m, n)."""
    m, n = V.shape[2:]
    _f64(V, (2, 2, m, n)), _f64(gamma, (2, m, n)), _f64(frames, (2, m, n)), _f64(grads, (2, 2, m, n))
    _lib.check(_lib.lib().psh_proesmans_sweep_dev(frames.ptr, grads.ptr, gamma.ptr, V.ptr, m, n, float(lam)),
               "psh_proesmans_sweep_dev")
    return V


def next_level(V_prev, m_next, n_next):
    """``_initialize_next_level``: (2, 2, m_next, n_next) from V_prev (2, 2, m_prev, n_prev)."""
    m_prev, n_prev = V_prev.shape[2:]
    _f64(V_prev, (2, 2, m_prev, n_prev))
    out = DeviceArray((2, 2, m_next, n_next), np.float64)
    _lib.check(_lib.lib().psh_proesmans_next_level_dev(V_prev.ptr, m_prev, n_prev, out.ptr, m_next, n_next),
               "psh_proesmans_next_level_dev")
    return out


def advection_field(scaled, lam, num_iter, num_levels, dtype=np.float64):
    """``_compute_advection_field`` on scaled frames (2, m, n) float64: (V (2, 2, m, n), GAMMA (2, m, n)) of ``dtype``."""
    m, n = scaled.shape[1:]
    _f64(scaled, (2, m, n))
    V = DeviceArray((2, 2, m, n), dtype)
    gamma = DeviceArray((2, m, n), dtype)
    _lib.check(_lib.lib().psh_proesmans_dev(scaled.ptr, m, n, float(lam), int(num_iter), int(num_levels),
                                            int(np.dtype(dtype) == np.float32), V.ptr, gamma.ptr), "psh_proesmans_dev")
    return V, gamma


def launches_per_iteration(m, n):
    """Kernel launches of one iteration at a (m, n) level: three for the consistency maps, the sweep's anti-diagonals
    and the edge fill."""
    return 3 + int(_lib.load().psh_proesmans_sweep_launches(int(m), int(n)))


def _unsupported(shape, num_levels):
    """Why the device path does not take this call (None if it does)."""
    m, n = int(shape[1]), int(shape[2])
    if int(num_levels) < 1:
        return "num_levels=%d" % num_levels
    for _ in range(1, int(num_levels)):
        m, n = m // 2, n // 2
    if m < 3 or n < 3:
        return "a coarsest pyramid level of %d x %d (each side must be at least 3)" % (m, n)
    return None


def _to_reference(why, input_images, kwargs):
    ref = lookup("motion.proesmans", "proesmans", proesmans)
    if ref is None:
        raise NotImplementedError("pysteps_amd proesmans: %s, and pysteps is not importable for the reference's proesmans"
                                  % why)
    warnings.warn("pysteps_amd proesmans: %s - running the reference's proesmans" % why, RuntimeWarning, stacklevel=3)
    resident = isinstance(input_images, DeviceArray)
    host = input_images.to_host() if resident else np.asarray(input_images)
    out = ref(host.astype(np.float64), **kwargs)
    if not resident:
        return out
    return tuple(DeviceArray.from_host(o) for o in out) if isinstance(out, tuple) else DeviceArray.from_host(out)


def proesmans(input_images, lam=50.0, num_iter=100, num_levels=6, filter_std=0.0, verbose=True, full_output=False):
    """Implementation of the anisotropic diffusion method of Proesmans et al. (1994) (reference:
    pysteps/motion/proesmans.py; keywords, defaults, checks and return value as documented there).

    ``input_images``: (2, m, n) NumPy array or DeviceArray.  Returns the forward advection field (2, m, n), or with
    ``full_output=True`` the forward-backward fields (2, 2, m, n) and the consistency maps (2, m, n).  NumPy input
    (float32 is widened; the reference rejects it) gives float64 NumPy output, a DeviceArray gives DeviceArrays, float32
    for float32 frames."""
    del verbose  # not used, as in the reference
    _check_input_frames(input_images)
    kwargs = dict(lam=lam, num_iter=num_iter, num_levels=num_levels, filter_std=filter_std, full_output=full_output)
    resident = isinstance(input_images, DeviceArray)
    why = _unsupported(input_images.shape, num_levels)
    if why is None and not resident and not np.all(np.isfinite(input_images)):
        why = "non-finite input values"
    if why is not None:
        return _to_reference(why, input_images, kwargs)

    if resident:
        frames = input_images
    else:
        arr = np.asarray(input_images)
        frames = DeviceArray.from_host(np.ascontiguousarray(arr, dtype=np.float32 if arr.dtype == np.float32 else np.float64))
    ev = [Event().record()]
    scaled, (_, _, nonfinite) = scale_frames(frames)
    if nonfinite:
        return _to_reference("non-finite input values", input_images, kwargs)
    ev.append(Event().record())
    if filter_std > 0.0:
        from scipy.ndimage import gaussian_filter  # noqa: PLC0415

        im = scaled.to_host()
        im[0, :, :] = gaussian_filter(im[0, :, :], filter_std)
        im[1, :, :] = gaussian_filter(im[1, :, :], filter_std)
        scaled = DeviceArray.from_host(im)
    ev.append(Event().record())
    m, n = scaled.shape[1:]
    dtype = np.float32 if resident and frames.dtype == np.float32 else np.float64
    V, gamma = advection_field(scaled, lam, num_iter, num_levels, dtype)
    ev.append(Event().record())
    synchronize()
    last_run_stats.clear()
    last_run_stats.update(scale=ev[0].elapsed_ms(ev[1]), filter=ev[1].elapsed_ms(ev[2]), flow=ev[2].elapsed_ms(ev[3]),
                          total=ev[0].elapsed_ms(ev[3]), launches_per_iteration=launches_per_iteration(m, n))
    if resident:
        return (V, gamma) if full_output else V.view(0)
    return (V.to_host(), gamma.to_host()) if full_output else V.view(0).to_host()
