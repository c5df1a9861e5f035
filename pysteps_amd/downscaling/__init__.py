"""Stochastic downscaling on the GPU: ``get_method("rainfarm_hip")``."""
from .interface import get_method  # noqa: F401
from .rainfarm import downscale, downscale_table  # noqa: F401
