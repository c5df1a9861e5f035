"""Mirrors of pysteps.postprocessing operators that sit inside the nowcast member loops, and the ensemble statistics
behind them; ``get_method`` mirrors pysteps/postprocessing/interface.py for the names this package serves."""

from . import probmatching  # noqa: F401
from .._registry import MethodTable

_table = MethodTable("ensemblestats")


def get_method(name):
    """The ensemble statistic registered under ``name``: ``"mean_hip"`` / ``"excprob_hip"``
    (:func:`pysteps_amd.postprocessing.ensemblestats.mean` / ``excprob``)."""
    if not _table.names():
        from . import ensemblestats  # noqa: PLC0415

        _table.add("mean_hip", ensemblestats.mean)
        _table.add("excprob_hip", ensemblestats.excprob)
    return _table.lookup(name)
