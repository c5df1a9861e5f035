"""Linear and salient blending of (ensemble) nowcasts with (ensemble) NWP forecasts on the device (mirror of
pysteps/blending/linear_blending.py), registered as ``"linear_blending_hip"`` and ``"salient_blending_hip"``.

:func:`forecast` has the reference's signature: it runs the nowcast (a method of :mod:`pysteps_amd.nowcasts` first, one
of pysteps' own table otherwise, whose host result is uploaded), converts both sides to rain rates and hands them to
:func:`blend`, the stage after the unit conversion.  Per lead time the device runs one pass (csrc/blending.hip):

* before ``start_blending`` a copy of the nowcast with its NaNs filled, after ``end_blending`` a copy of the NWP read
  through ``np.nan_to_num(nan=0.0)``, in between ``weight_nwp * nwp + weight_nowcast * nowcast`` with NumPy's
  arithmetic - each product in its array's dtype with the Python-float weight rounded to it, the sum in the common
  dtype, rounded once to the NWP's dtype at the store, no fused multiply-add;
* with ``saliency=True`` the maxima and the dense ranks of ``nowcast / max - nwp / max`` over all members of the lead
  time jointly (the reference hands ``_get_ranked_salience`` the slice ``[:, i]``), by a radix sort of
  order-preserving integer keys, then the reference's ``_get_ws`` in its written order in float64.

The weights are computed here exactly as the reference computes them and passed as doubles.  The pairing of nowcast
members with NWP members is a host index map (:func:`member_maps`); repeated members are never materialised.  A host
NWP stack is uploaded one lead time at a time, and only the lead times that are read.  Everything the device computes
is made of correctly rounded IEEE operations and integer ranks, so the result is the reference's bit for bit.

A ``DeviceArray`` ``precip`` gives a ``DeviceArray``, host input an ``ndarray``; inputs are never modified.  Declined:
units other than ``"mm/h"`` / ``"mm"``, transforms other than ``None`` / ``"dB"``, dtypes other than float32 /
float64, shapes ``np.squeeze`` would change beyond the member axis, and a salient lead time whose maximum is not
finite - host callers get the reference's function with a ``RuntimeWarning``, resident callers ``NotImplementedError``.
"""

import ctypes

import numpy as np

from .. import _lib
from .._reference import decline, lookup
from .._reference import method as reference_method
from ..device import DeviceArray
from ..utils.transformation import _transform_dev

__all__ = ["forecast", "blend", "weight_schedule", "member_maps", "to_rainrate"]

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


class _Declined(Exception):
    """Input the device path does not take; carries the reason."""


def weight_schedule(timesteps, timestep, start_blending, end_blending):
    """``weight_nwp`` of every lead time as the reference computes and clamps it (linear_blending.py:215-239)."""
    weights = []
    for i in range(timesteps):
        t = (i + 1) * timestep
        weight_nwp = (t - start_blending) / (end_blending - start_blending)
        if weight_nwp <= 0.0:
            weight_nwp = 0.0
        elif weight_nwp >= 1.0:
            weight_nwp = 1.0
        weights.append(weight_nwp)
    return weights


def member_maps(n_nowcast, n_nwp):
    """``(map_nowcast, map_nwp)``: the member of either side that output member k is made of - the reference's
    ``np.repeat`` of the shorter ensemble (linear_blending.py:163-184) as an index map."""
    n_max, n_min = max(n_nowcast, n_nwp), min(n_nowcast, n_nwp)
    full = np.arange(n_max, dtype=np.int64)
    if n_min == n_max:
        return full, full.copy()
    if n_min == 1:
        short = np.zeros(n_max, dtype=np.int64)
    else:
        repeats = [(n_max + i) // n_min for i in range(n_min)]
        short = np.repeat(np.arange(n_min, dtype=np.int64), repeats)
    return (full, short) if n_nwp == n_min else (short, full)


def _unit_problem(metadata, what):
    """Why the device does not convert these units (None if it does)."""
    if metadata["transform"] not in (None, "dB"):
        return "the %s transform %r" % (what, metadata["transform"])
    if metadata["unit"] not in ("mm/h", "mm"):
        return "the %s unit %r" % (what, metadata["unit"])
    return None


def to_rainrate(field, metadata):
    """The reference's ``conversion.to_rainrate`` of a float32 / float64 DeviceArray for the units the device serves:
    the inverse dB transform, then ``/ accutime * 60.0`` for accumulations.  Returns ``field`` itself when there is
    nothing to convert; never writes into it."""
    why = _unit_problem(metadata, "field's")
    if why is not None or field.dtype not in _FLOATS:
        raise NotImplementedError("pysteps_amd blending: %s is not converted on the device" % (why or "dtype %s" % field.dtype))
    lib = _lib.lib()
    out = field
    if metadata["transform"] == "dB":
        if field.dtype == np.float32:
            out = _transform_dev(field, 10.0 ** (metadata.get("threshold", -10.0) / 10.0), 0.0, True)
        else:
            out = DeviceArray(field.shape, field.dtype)
            _lib.check(lib.psh_blend_db_inverse_f64_dev(field.ptr, out.ptr, field.size,
                                                        float(metadata.get("threshold", -10.0)), 0.0),
                       "psh_blend_db_inverse_f64_dev")
    if metadata["unit"] == "mm":
        src = out
        if out is field:
            out = DeviceArray(field.shape, field.dtype)
        _lib.check(lib.psh_blend_scale_dev(src.ptr, out.ptr, int(field.dtype == np.float32), field.size,
                                           float(metadata["accutime"]), 60.0), "psh_blend_scale_dev")
    return out


def _stack_shape(x, what):
    """(K, T, m, n) of a (t, m, n) or (K, t, m, n) stack, as the reference reads it."""
    shape = tuple(int(s) for s in x.shape)
    if x.dtype not in _FLOATS:
        raise _Declined("a %s of dtype %s" % (what, x.dtype))
    if len(shape) == 3:
        shape = (1,) + shape
    elif len(shape) != 4:
        raise _Declined("a %d-dimensional %s" % (len(shape), what))
    elif shape[0] == 1 and 1 in shape[1:]:
        raise _Declined("a single-member %s with another axis of length 1 (np.squeeze removes it)" % what)
    if 1 in shape[2:]:
        raise _Declined("a %s with a spatial side of 1" % what)
    if 0 in shape:
        raise _Declined("an empty %s" % what)
    return shape


def _blend(precip_nowcast, precip_nwp, nwp_metadata, timesteps, timestep, start_blending, end_blending, fill_nwp, saliency):
    """The blend of a rain-rate nowcast DeviceArray with an NWP stack (host or device, converted with ``nwp_metadata``
    when one is given).  Returns the DeviceArray of the result; raises :class:`_Declined`."""
    timesteps_nowcast = int(end_blending / timestep)
    Kn, Tn, m, n = _stack_shape(precip_nowcast, "nowcast")
    nwp_resident = isinstance(precip_nwp, DeviceArray)
    if not nwp_resident:
        precip_nwp = np.asarray(precip_nwp)
    Kw, Tw, mw, nw = _stack_shape(precip_nwp, "NWP stack")
    T = min(Tw, timesteps)  # precip_nwp[..., 0:timesteps, :, :]
    assert (mw, nw) == (m, n), (
        "The x and y dimensions of precip_nowcast and precip_nwp need to be identical: dimension of precip_nwp = {} "
        "and dimension of precip_nowcast = {}".format((mw, nw), (m, n)))
    K = max(Kn, Kw)
    # the reference's boolean index of the NaN fill and its loop over range(timesteps) raise IndexError otherwise
    if min(T, timesteps_nowcast) != Tn:
        raise IndexError("boolean index did not match indexed array: the NWP stack holds %d of the nowcast's %d lead times"
                         % (min(T, timesteps_nowcast), Tn))
    if timesteps > T:
        raise IndexError("index %d is out of bounds for the NWP stack's time axis with size %d" % (T, T))
    weights = weight_schedule(timesteps, timestep, start_blending, end_blending)
    if any(w < 1.0 for w in weights[Tn:]):
        raise IndexError("index %d is out of bounds for the nowcast's time axis with size %d" % (Tn, Tn))
    map_n, map_w = member_maps(Kn, Kw)
    plane = m * n
    nwp_dtype = precip_nwp.dtype
    convert = nwp_metadata is not None and (nwp_metadata["transform"] is not None or nwp_metadata["unit"] != "mm/h")
    if nwp_resident and convert:
        precip_nwp = to_rainrate(precip_nwp, nwp_metadata)

    out = DeviceArray((T, m, n) if K == 1 else (K, T, m, n), nwp_dtype)
    offsets = np.zeros((timesteps, 3, K), dtype=np.int64)
    lead = np.arange(timesteps, dtype=np.int64)[:, None]
    offsets[:, 0, :] = np.where(lead < Tn, (map_n[None, :] * Tn + lead) * plane, 0)
    offsets[:, 1, :] = (map_w[None, :] * Tw + lead) * plane if nwp_resident else map_w[None, :] * plane
    offsets[:, 2, :] = (np.arange(K, dtype=np.int64)[None, :] * T + lead) * plane
    d_offsets = DeviceArray.from_host(offsets)
    lib = _lib.lib()
    nc_f32, nwp_f32 = int(precip_nowcast.dtype == np.float32), int(nwp_dtype == np.float32)
    host_nwp = None if nwp_resident else precip_nwp.reshape(Kw, Tw, m, n)
    status = ctypes.c_int(0)
    for i, weight_nwp in enumerate(weights):
        mode = 0 if weight_nwp == 0.0 else (1 if weight_nwp == 1.0 else 2)
        nwp_read = mode != 0 or (fill_nwp and i < Tn)
        nwp_lead = precip_nwp if nwp_resident else None
        if nwp_read and not nwp_resident:
            nwp_lead = DeviceArray.from_host(np.ascontiguousarray(host_nwp[:, i]))
            if convert:
                nwp_lead = to_rainrate(nwp_lead, nwp_metadata)
        off_ptr = d_offsets.ptr + i * 3 * K * 8
        nwp_ptr = nwp_lead.ptr if nwp_read else None
        if mode == 2 and saliency:
            weight = 1.0 - weight_nwp
            _lib.check(lib.psh_blend_salient_dev(precip_nowcast.ptr, nc_f32, nwp_ptr, nwp_f32, off_ptr, K, plane, weight,
                                                 1 - weight, weight**2, (1 - weight) ** 2, int(bool(fill_nwp)), out.ptr,
                                                 ctypes.byref(status), None), "psh_blend_salient_dev")
            if status.value:
                raise _Declined("a salient lead time whose %s" % ("maximum is not finite" if status.value & 1
                                                                 else "normalised difference is NaN"))
        else:
            _lib.check(lib.psh_blend_linear_dev(precip_nowcast.ptr if mode != 1 else None, nc_f32, nwp_ptr, nwp_f32, off_ptr, K,
                                                plane, mode, weight_nwp, 1.0 - weight_nwp, int(bool(fill_nwp)), out.ptr),
                       "psh_blend_linear_dev")
    return out


def blend(precip_nowcast, precip_nwp, timesteps, timestep, start_blending, end_blending, fill_nwp=True, saliency=False):
    """The reference's ``forecast`` after the unit conversion (linear_blending.py:134-260): ``precip_nowcast``
    ``(int(end_blending / timestep), m, n)`` or ``(K, ., m, n)`` and ``precip_nwp`` ``(t, m, n)`` or ``(K', t, m, n)``
    in mm/h, float32 or float64, NumPy arrays or DeviceArrays -> the blended stack shaped like the (member-repeated)
    NWP stack cut to ``timesteps``, in the NWP's dtype.  A DeviceArray nowcast gives a DeviceArray.  Input this stage
    does not take raises ``NotImplementedError``."""
    resident = isinstance(precip_nowcast, DeviceArray)
    nowcast = precip_nowcast if resident else DeviceArray.from_host(np.ascontiguousarray(precip_nowcast))
    try:
        out = _blend(nowcast, precip_nwp, None, timesteps, timestep, start_blending, end_blending, fill_nwp, saliency)
    except _Declined as exc:
        decline("blending", str(exc), None, resident)
    return out if resident else out.to_host()


def _nowcast_method(name):
    """``(method, ours)``: the nowcast of :mod:`pysteps_amd.nowcasts`, else the one of pysteps' table."""
    from .. import nowcasts  # noqa: PLC0415

    try:
        return nowcasts.get_method(name), True
    except ValueError:
        return reference_method("nowcasts", name), False


def _host(x):
    return x.to_host() if isinstance(x, DeviceArray) else x


def _forecast(precip, precip_metadata, velocity, timesteps, timestep, nowcast_method, precip_nwp, precip_nwp_metadata,
              start_blending, end_blending, fill_nwp, saliency, nowcast_kwargs):
    if len(precip.shape) == 3:
        precip = precip.view(precip.shape[0] - 1) if isinstance(precip, DeviceArray) else precip[-1, :, :]
    timesteps_nowcast = int(end_blending / timestep)
    why = _unit_problem(precip_metadata, "nowcast's")
    if why is None and precip_nwp is not None:
        why = _unit_problem(precip_nwp_metadata, "NWP's")
    if why is not None:
        raise _Declined(why)
    if precip_nwp is not None and len(precip_nwp.shape) in (3, 4):
        nwp_steps = min(int(precip_nwp.shape[-3]), timesteps)
        if nwp_steps < timesteps_nowcast:  # the reference's NaN fill fails on its boolean index; no device work before
            raise IndexError("boolean index did not match indexed array: the NWP stack holds %d of the nowcast's %d lead times"
                             % (nwp_steps, timesteps_nowcast))
    method, ours = _nowcast_method(nowcast_method)
    steps =timesteps_nowcast if precip_nwp is not None else timesteps
    if ours:
        # the device nowcasts take their inputs from one side: the velocity follows precip
        if isinstance(precip, DeviceArray) and not isinstance(velocity, DeviceArray):
            velocity = DeviceArray.from_host(np.ascontiguousarray(velocity, dtype=np.float32))
        elif not isinstance(precip, DeviceArray):
            velocity = _host(velocity)
        nowcast = method(precip, velocity, steps, **nowcast_kwargs)
    else:
        nowcast = method(_host(precip), _host(velocity), steps, **nowcast_kwargs)
    if not isinstance(nowcast, DeviceArray):
        nowcast = DeviceArray.from_host(np.ascontiguousarray(nowcast))
    if nowcast.dtype not in _FLOATS:
        raise _Declined("a nowcast of dtype %s" % nowcast.dtype)
    nowcast = to_rainrate(nowcast, precip_metadata)
    if precip_nwp is None:
        return nowcast
    return _blend(nowcast, precip_nwp, precip_nwp_metadata, timesteps, timestep, start_blending, end_blending, fill_nwp, saliency)


def forecast(precip, precip_metadata, velocity, timesteps, timestep, nowcast_method, precip_nwp=None,
             precip_nwp_metadata=None, start_blending=120, end_blending=240, fill_nwp=True, saliency=False,
             nowcast_kwargs=None):
    """Generate a forecast by linearly or saliency-based blending of nowcasts with NWP data (reference:
    pysteps/blending/linear_blending.py ``forecast``; arguments and return value as documented there).

    ``precip``, ``velocity`` and ``precip_nwp`` may each be a NumPy array or a DeviceArray; a DeviceArray ``precip``
    gives a DeviceArray.  ``nowcast_method`` is looked up in :func:`pysteps_amd.nowcasts.get_method` first and in
    pysteps' table otherwise."""
    if nowcast_kwargs is None:
        nowcast_kwargs = dict()
    resident = isinstance(precip, DeviceArray)
    try:
        out = _forecast(precip, precip_metadata, velocity, timesteps, timestep, nowcast_method, precip_nwp,
                        precip_nwp_metadata, start_blending, end_blending, fill_nwp, saliency, nowcast_kwargs)
    except _Declined as exc:
        reference = decline("blending", str(exc), lookup("blending.linear_blending", "forecast", forecast), resident)
        return reference(precip, precip_metadata, _host(velocity), timesteps, timestep, nowcast_method,
                         precip_nwp=None if precip_nwp is None else _host(precip_nwp),
                         precip_nwp_metadata=precip_nwp_metadata, start_blending=start_blending, end_blending=end_blending,
                         fill_nwp=fill_nwp, saliency=saliency, nowcast_kwargs=nowcast_kwargs)
    return out if resident else out.to_host()
