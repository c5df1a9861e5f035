"""Callers of the advection operators that are thin enough to mirror, and the nowcasts that
run on the device; ``get_method`` mirrors pysteps/nowcasts/interface.py for the names this package serves."""

from .._registry import MethodTable

_table = MethodTable("nowcast")


def get_method(name):
    """The nowcast registered under ``name``: ``"anvil_hip"`` (:func:`pysteps_amd.nowcasts.anvil.forecast`),
    ``"lagrangian_probability_hip"`` (:func:`pysteps_amd.nowcasts.lagrangian_probability.forecast`),
    ``"extrapolation"`` / ``"lagrangian"`` (:func:`pysteps_amd.nowcasts.extrapolation.forecast`)."""
    if not _table.names():
        from . import anvil, extrapolation, lagrangian_probability  # noqa: PLC0415

        _table.add("anvil_hip", anvil.forecast)
        _table.add("lagrangian_probability_hip", lagrangian_probability.forecast)
        _table.add(["extrapolation", "lagrangian"], extrapolation.forecast)
    return _table.lookup(name)
