"""``downscaling.get_method`` mirror (reference: pysteps/downscaling/interface.py).

"rainfarm" and "rainfarm_hip" resolve to the HIP RainFARM (:func:`pysteps_amd.downscaling.rainfarm.downscale`).
"""

from .._registry import MethodTable
from .rainfarm import downscale

_table = MethodTable("downscaling")
_table.add(["rainfarm", "rainfarm_hip"], downscale)


def get_method(name):
    """Return the downscaling callable registered under ``name``."""
    return _table.lookup(name)
