"""Mirrors of pysteps.verification scores that run on the device; ``get_method`` mirrors
pysteps/verification/interface.py for the names this package serves."""

from . import detcatscores, detcontscores, ensscores, probscores, spatialscores  # noqa: F401
from .._registry import MethodTable
from .detcatscores import (det_cat_fct, det_cat_fct_accum, det_cat_fct_compute, det_cat_fct_init, det_cat_fct_merge,  # noqa: F401
                           det_cat_table)
from .detcontscores import (det_cont_fct, det_cont_fct_accum, det_cont_fct_compute, det_cont_fct_init,  # noqa: F401
                            det_cont_fct_merge, det_cont_table)
from .detscores import DetScoresAccumulator  # noqa: F401
from .ensscores import SpreadSkillAccumulator, ensemble_skill, ensemble_spread, pair_scores  # noqa: F401
from .probscores import (CRPS, CRPS_accum, CRPS_compute, CRPS_init, ProbScoresAccumulator, ROC_curve, ROC_curve_accum,  # noqa: F401
                         ROC_curve_compute, ROC_curve_init, crps_table, reldiag, reldiag_accum, reldiag_compute, reldiag_init)
from .spatialscores import FssAccumulator, fss, fss_accum, fss_compute, fss_init, fss_merge, fss_table  # noqa: F401

# the score names the reference's get_method answers with det_cat_fct / det_cont_fct (interface.py:173-213)
CATEGORICAL_SCORES = ("acc", "bias", "csi", "f1", "fa", "far", "gss", "hk", "hss", "mcc", "pod", "sedi")
CONTINUOUS_SCORES = ("beta", "beta1", "beta2", "corr_p", "corr_s", "drmse", "mae", "mse", "me", "nmse", "rmse", "rv", "scatter")


def _categorical(name):
    def f(fct, obs, **kwargs):
        return detcatscores.det_cat_fct(fct, obs, kwargs.pop("thr"), [name])

    return f


def _continuous(name):
    def f(fct, obs, **kwargs):
        return detcontscores.det_cont_fct(fct, obs, [name], **kwargs)

    return f


_table = MethodTable("verification")
_table.add("fss", spatialscores.fss)
_table.add("det_cat_fct", detcatscores.det_cat_fct)
_table.add("det_cont_fct", detcontscores.det_cont_fct)
for _name in CATEGORICAL_SCORES:
    _table.add(_name, _categorical(_name))
for _name in CONTINUOUS_SCORES:
    _table.add(_name, _continuous(_name))


_PROBABILISTIC = {"crps": probscores.CRPS, "reldiag": probscores.reldiag, "roc": probscores.ROC_curve}


def get_method(name, type="deterministic"):  # noqa: A002 (the reference's parameter name)
    """The verification score registered under ``name``, as in the reference's ``get_method(name, type)``.
    ``type="deterministic"``: ``"fss"`` (:func:`pysteps_amd.verification.spatialscores.fss`), ``"det_cat_fct"`` and
    ``"det_cont_fct"`` themselves, and the score names the reference answers with them - a categorical name gives
    ``f(fct, obs, thr=...)``, a continuous one ``f(fct, obs, **kwargs)``, each returning the one-score dict.
    ``type="probabilistic"``: ``"crps"``, ``"reldiag"`` and ``"roc"`` (:mod:`pysteps_amd.verification.probscores`
    ``CRPS``, ``reldiag``, ``ROC_curve``)."""
    if isinstance(type, str) and type.lower() == "probabilistic":
        try:
            return _PROBABILISTIC[(name or "none").lower()]
        except KeyError:
            raise ValueError("unknown probabilistic method %s" % name) from None
    if isinstance(type, str) and type.lower() != "deterministic":
        raise ValueError("Unknown verification type %s\nThe available types are: ['deterministic', 'probabilistic']" % type)
    return _table.lookup(name)
