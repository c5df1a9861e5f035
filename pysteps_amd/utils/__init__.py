"""Sparse-vector utilities on the dense-LK path (mirrors of pysteps.utils.cleansing / interpolate), the transforms, the
unit conversions and the aggregation / clipping / squaring of pysteps.utils.dimension."""

from .cleansing import decluster, detect_outliers, detect_outliers_device  # noqa: F401
from .interpolate import idwinterp2d, rbfinterp2d  # noqa: F401
from .transformation import NQ_transform, boxcox_transform, dB_transform, sqrt_transform  # noqa: F401,E402
from .conversion import to_raindepth, to_rainrate, to_reflectivity  # noqa: F401,E402
from .check_norain import check_norain  # noqa: F401,E402
from .spectral import RapsdAccumulator, rapsd, rapsd_counts, rapsd_table  # noqa: F401,E402
from .dimension import (  # noqa: F401,E402
    TimeAggregator, aggregate_fields, aggregate_fields_space, aggregate_fields_time, clip_domain, square_domain,
)

# transformation, conversion and dimension names of pysteps/utils/interface.py, served from this package
_METHODS = {
    "accumulate": aggregate_fields_time,
    "clip": clip_domain,
    "square": square_domain,
    "upscale": aggregate_fields_space,
    "mm/h": to_rainrate, "rainrate": to_rainrate,
    "mm": to_raindepth, "raindepth": to_raindepth,
    "dbz": to_reflectivity, "reflectivity": to_reflectivity,
    "boxcox": boxcox_transform, "box-cox": boxcox_transform, "log": boxcox_transform,
    "db": dB_transform, "decibel": dB_transform,
    "nqt": NQ_transform,
    "sqrt": sqrt_transform,
}


def get_method(name, **kwargs):
    """``pysteps.utils.get_method``: the transformation, conversion and dimension methods come from this package, every
    other name from the reference's table.  ``None`` is "none", names are matched in lower case."""
    if name is None:
        name = "none"
    name = name.lower()
    if name in _METHODS:
        return _METHODS[name]
    import importlib

    return importlib.import_module("pysteps.utils").get_method(name, **kwargs)
