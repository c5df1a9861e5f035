"""Unit conversions, mirror of pysteps/utils/conversion.py (``to_rainrate``, ``to_raindepth``, ``to_reflectivity``).

Each function first undoes ``metadata["transform"]`` through the matching inverse of :mod:`.transformation`, then converts
by unit with the threshold and the zerovalue converted alongside.  NumPy input runs the reference's NumPy operations on
the host; a :class:`~pysteps_amd.device.DeviceArray` goes through ``psh_field_transform_dev`` (the Z-R power laws) and
``psh_blend_scale_dev`` (the accumulation scalings, two correctly rounded operations in the field's dtype) and never
touches the host.
"""

import numpy as np

from .. import _lib
from ..device import DeviceArray
from . import transformation

__all__ = ["to_rainrate", "to_raindepth", "to_reflectivity"]


def _untransform(R, metadata):
    name = metadata["transform"]
    if name is None:
        return R, metadata
    if name == "dB":
        return transformation.dB_transform(R, metadata, inverse=True)
    if name in ["BoxCox", "log"]:
        return transformation.boxcox_transform(R, metadata, inverse=True)
    if name == "NQT":
        return transformation.NQ_transform(R, metadata, inverse=True)
    if name == "sqrt":
        return transformation.sqrt_transform(R, metadata, inverse=True)
    raise ValueError("Unknown transformation %s" % name)


def _start(R, metadata):
    metadata = metadata.copy()
    if not isinstance(R, DeviceArray):
        R = R.copy()
    return _untransform(R, metadata)


def _scale(R, divisor, factor):
    """``R / divisor * factor``: each operation rounded in the field's dtype."""
    if not isinstance(R, DeviceArray):
        return R / divisor * factor
    transformation._resident_real("conversion", R, divisor, factor)
    out = DeviceArray(R.shape, R.dtype)
    _lib.check(_lib.lib().psh_blend_scale_dev(R.ptr, out.ptr, int(R.dtype == np.float32), R.size, float(divisor), float(factor)),
               "psh_blend_scale_dev")
    return out


def _zr(metadata, zr_a, zr_b):
    if zr_a is None:
        zr_a = metadata.get("zr_a", 200.0)  # Marshall-Palmer
    if zr_b is None:
        zr_b = metadata.get("zr_b", 1.6)
    return zr_a, zr_b


def _z_to_rate(R, zr_a, zr_b):
    if not isinstance(R, DeviceArray):
        return (R / zr_a) ** (1.0 / zr_b)
    transformation._resident_real("conversion", R, zr_a, zr_b)
    return transformation._pass_dev(R, transformation.OP_Z_TO_RATE, zr_a, 1.0 / zr_b)


def _rate_to_z(R, zr_a, zr_b):
    if not isinstance(R, DeviceArray):
        return zr_a * R ** zr_b
    transformation._resident_real("conversion", R, zr_a, zr_b)
    return transformation._pass_dev(R, transformation.OP_RATE_TO_Z, zr_a, zr_b)


def to_rainrate(R, metadata, zr_a=None, zr_b=None):
    """Convert to rain rate [mm/h]; parameters, return value and metadata updates of the reference (conversion.py:25-113)."""
    R, metadata = _start(R, metadata)
    unit = metadata["unit"]
    if unit == "mm/h":
        pass
    elif unit == "mm":
        accutime = float(metadata["accutime"])
        R = _scale(R, accutime, 60.0)
        metadata["threshold"] = metadata["threshold"] / accutime * 60.0
        metadata["zerovalue"] = metadata["zerovalue"] / accutime * 60.0
    elif unit == "dBZ":
        threshold, zerovalue = metadata["threshold"], metadata["zerovalue"]
        zr_a, zr_b = _zr(metadata, zr_a, zr_b)
        R = _z_to_rate(R, zr_a, zr_b)
        metadata["zr_a"] = zr_a
        metadata["zr_b"] = zr_b
        metadata["threshold"] = (threshold / zr_a) ** (1.0 / zr_b)
        metadata["zerovalue"] = (zerovalue / zr_a) ** (1.0 / zr_b)
    else:
        raise ValueError("Cannot convert unit %s and transform %s to mm/h" % (unit, metadata["transform"]))
    metadata["unit"] = "mm/h"
    return R, metadata


def to_raindepth(R, metadata, zr_a=None, zr_b=None):
    """Convert to rain depth [mm]; parameters, return value and metadata updates of the reference (conversion.py:116-204)."""
    R, metadata = _start(R, metadata)
    unit = metadata["unit"]
    if unit == "mm" and metadata["transform"] is None:
        pass
    elif unit == "mm/h":
        accutime = metadata["accutime"]
        R = _scale(R, 60.0, accutime)
        metadata["threshold"] = metadata["threshold"] / 60.0 * accutime
        metadata["zerovalue"] = metadata["zerovalue"] / 60.0 * accutime
    elif unit == "dBZ":
        threshold, zerovalue = metadata["threshold"], metadata["zerovalue"]
        accutime = metadata["accutime"]
        zr_a, zr_b = _zr(metadata, zr_a, zr_b)
        R = _scale(_z_to_rate(R, zr_a, zr_b), 60.0, accutime)
        metadata["zr_a"] = zr_a
        metadata["zr_b"] = zr_b
        metadata["threshold"] = (threshold / zr_a) ** (1.0 / zr_b) / 60.0 * accutime
        metadata["zerovalue"] = (zerovalue / zr_a) ** (1.0 / zr_b) / 60.0 * accutime
    else:
        raise ValueError("Cannot convert unit %s and transform %s to mm" % (unit, metadata["transform"]))
    metadata["unit"] = "mm"
    return R, metadata


def to_reflectivity(R, metadata, zr_a=None, zr_b=None):
    """Convert to reflectivity [dBZ]; parameters, return value and metadata updates of the reference
    (conversion.py:207-299)."""
    R, metadata = _start(R, metadata)
    unit = metadata["unit"]
    if unit in ("mm/h", "mm"):
        if unit == "mm":
            R, metadata = to_rainrate(R, metadata)
        zr_a, zr_b = _zr(metadata, zr_a, zr_b)
        R = _rate_to_z(R, zr_a, zr_b)
        metadata["threshold"] = zr_a * metadata["threshold"] ** zr_b
        metadata["zerovalue"] = zr_a * metadata["zerovalue"] ** zr_b
        metadata["zr_a"] = zr_a
        metadata["zr_b"] = zr_b
        R, metadata = transformation.dB_transform(R, metadata)
    elif unit == "dBZ":
        R, metadata = transformation.dB_transform(R, metadata)
    else:
        raise ValueError("Cannot convert unit %s and transform %s to mm/h" % (unit, metadata["transform"]))
    metadata["unit"] = "dBZ"
    return R, metadata
