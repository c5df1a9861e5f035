"""Blending of nowcasts with NWP forecasts on the device (mirror of ``pysteps.blending`` for the linear and the salient
method)."""

from .interface import get_method  # noqa: F401
