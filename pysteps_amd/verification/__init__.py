"""Mirrors of pysteps.verification scores that run on the device; ``get_method`` mirrors
pysteps/verification/interface.py for the names this package serves."""

from . import spatialscores  # noqa: F401
from .._registry import MethodTable
from .spatialscores import FssAccumulator, fss, fss_accum, fss_compute, fss_init, fss_merge, fss_table  # noqa: F401

_table = MethodTable("verification")
_table.add("fss", spatialscores.fss)


def get_method(name, type="deterministic"):  # noqa: A002 (the reference's parameter name)
    """The verification score registered under ``name``: ``"fss"`` (:func:`pysteps_amd.verification.spatialscores.fss`,
    a deterministic score as in the reference's ``get_method(name, type="deterministic")``)."""
    if isinstance(type, str) and type.lower() != "deterministic":
        raise ValueError("Unknown verification type %s\nThe available types are: ['deterministic']" % type)
    return _table.lookup(name)
