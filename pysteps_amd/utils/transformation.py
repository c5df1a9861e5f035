"""dB transform on the device, mirror of pysteps/utils/transformation.py:150-232 (``dB_transform``).

NumPy inputs are transformed on the host exactly like the reference does (it is one
element-wise pass); :class:`~pysteps_amd.device.DeviceArray` inputs stay in HBM
(``psh_db_transform_dev``) so that rain rate -> dB -> LK -> extrapolation -> rain rate
never crosses PCIe.
"""

import ctypes

import numpy as np

from .. import _lib
from ..device import DeviceArray, _compared_as

__all__ = ["dB_transform", "field_stats", "field_nanmin"]


def _require_float32(field):
    if field.dtype != np.float32:
        raise ValueError("device-resident fields must be float32")


def _field_stats(field):
    _require_float32(field)
    mn, mx, bad, low = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    _lib.check(
        _lib.lib().psh_field_stats_dev(field.ptr, field.size, ctypes.byref(mn), ctypes.byref(mx), ctypes.byref(bad),
                                       ctypes.byref(low)),
        "psh_field_stats_dev",
    )
    return mn.value, mx.value, int(bad.value), low.value


def field_stats(field):
    """(min, max, number of non-finite values) of a float32 DeviceArray, computed on the device;
    min and max are over the finite values."""
    return _field_stats(field)[:3]


def field_nanmin(field):
    """``np.nanmin`` of a float32 DeviceArray from the same device reduction: NaNs are ignored, an
    infinity is a value (semilagrangian.py:171-172, outval="min")."""
    return _field_stats(field)[3]


def _transform_dev(R, compared_with, zerovalue, inverse):
    """One resident pass.  ``compared_with`` is the threshold object of the reference's ``<``, in the
    units of the values it is compared with; it decides in float32 or in float64 as NumPy would."""
    _require_float32(R)
    out = DeviceArray(R.shape, np.float32)
    _lib.check(_lib.lib().psh_db_transform_dev(R.ptr, out.ptr, R.size, _compared_as(compared_with, np.float32),
                                               float(zerovalue), int(inverse)), "psh_db_transform_dev")
    return out


def dB_transform(R, metadata=None, threshold=None, zerovalue=None, inverse=False):
    """Methods to transform precipitation intensities to/from dB units.

    Same parameters, return value ``(R, metadata)`` and metadata updates as the
    reference (transformation.py:150-232).
    """
    if metadata is None:
        metadata = {"transform": "dB"} if inverse else {"transform": None}
    else:
        metadata = metadata.copy()
    on_device = isinstance(R, DeviceArray)

    if not inverse:
        if metadata["transform"] == "dB":
            return (R if on_device else R.copy()), metadata
        if threshold is None:
            threshold = metadata.get("threshold", 0.1)
        threshold_db = 10.0 * np.log10(threshold)
        if zerovalue is None:
            zerovalue = threshold_db - 5
        if on_device:
            out = _transform_dev(R, threshold, zerovalue, False)
        else:
            out = R.copy()
            zeros = out < threshold
            out[~zeros] = 10.0 * np.log10(out[~zeros])
            out[zeros] = zerovalue
        metadata["transform"] = "dB"
        metadata["zerovalue"] = zerovalue
        metadata["threshold"] = threshold_db
        return out, metadata

    if metadata["transform"] != "dB":
        return (R if on_device else R.copy()), metadata
    if threshold is None:
        threshold = metadata.get("threshold", -10.0)
    if zerovalue is None:
        zerovalue = 0.0
    # formed as the reference forms it (:227), so it keeps the NumPy type that decides the comparison: the
    # metadata of a forward transform holds a numpy.float64, a Python float stays a Python float
    threshold_lin = 10.0 ** (threshold / 10.0)
    if on_device:
        out = _transform_dev(R, threshold_lin, zerovalue, True)
    else:
        out = 10.0 ** (R / 10.0)
        out[out < threshold_lin] = zerovalue
    metadata["transform"] = None
    metadata["threshold"] = threshold_lin
    metadata["zerovalue"] = zerovalue
    return out, metadata
