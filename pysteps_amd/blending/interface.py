"""``blending.get_method`` mirror (reference: pysteps/blending/interface.py).

"linear_blending" and "linear_blending_hip" resolve to :func:`pysteps_amd.blending.linear_blending.forecast`,
"salient_blending" and "salient_blending_hip" to the same function with ``saliency=True``.
"""

from functools import partial

from .._registry import MethodTable
from .linear_blending import forecast

_table = MethodTable("blending")
_table.add(["linear_blending", "linear_blending_hip"], forecast)
_table.add(["salient_blending", "salient_blending_hip"], partial(forecast, saliency=True))


def get_method(name):
    """Return the blending callable registered under ``name``."""
    return _table.lookup(name)
