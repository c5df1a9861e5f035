"""Mirrors of pysteps.timeseries operators that sit inside the nowcast member loops or in front of them."""

from . import autoregression, correlation  # noqa: F401
