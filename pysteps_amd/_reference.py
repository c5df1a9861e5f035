"""The reference's functions: where an operator finds the one to hand declined input to, and the table by which
``register`` swaps ours into pysteps' module attributes.  The only module, next to ``register`` and the ``get_method``
mirrors, that imports pysteps.

A swap parks the stock function on the reference's own module as ``_reference_<name>`` and :func:`lookup` reads it from
there, so no module of ours holds a reference function of its own.  :func:`lookup` is called once a call has been
declined, never at import time and never for a call the device takes.
"""

import importlib
import warnings


def lookup(module, name, ours):
    """The reference's ``pysteps.<module>.<name>`` - the parked ``_reference_<name>`` while a swap is in place - or None
    when pysteps, that submodule or that attribute is not importable, or when what is found there is ``ours``."""
    try:
        mod = importlib.import_module("pysteps." + module)
        fn = getattr(mod, "_reference_" + name, None) or getattr(mod, name)
    except Exception:
        return None
    return None if fn is ours else fn


def require(module, name, ours):
    """:func:`lookup` for a call that cannot go on without the reference's function: the import's own error when
    pysteps is absent, ``NotImplementedError`` when what is found is ``ours``."""
    fn = lookup(module, name, ours)
    if fn is None:
        importlib.import_module("pysteps." + module)
        raise NotImplementedError("the reference's %s is not reachable" % name)
    return fn


def method(package, name):
    """``pysteps.<package>.get_method(name)``: a method this package does not serve, from the reference's own table
    (the import's own error when pysteps is absent)."""
    return importlib.import_module("pysteps." + package).get_method(name)


def _is_fn(obj, module_suffix, name):
    """``obj`` is the function ``name`` of a module ending in ``module_suffix`` (the reference's or ours)."""
    return callable(obj) and getattr(obj, "__name__", "") == name and getattr(obj, "__module__", "").endswith(module_suffix)


def decline(name, why, reference, resident, category=RuntimeWarning):
    """Warn and return the reference's function for declined input, or raise when there is none to hand it to."""
    if reference is None or resident:
        raise NotImplementedError("pysteps_amd %s: %s is not implemented on the device%s"
                                  % (name, why, "" if reference is not None else " and pysteps is not importable"))
    warnings.warn("pysteps_amd %s: %s - running the reference's function" % (name, why), category, stacklevel=3)
    return reference


# What ``register`` swaps: (key, reference module, names, label prefix).  Our module has the same path under
# pysteps_amd; a string in place of the names is the tuple of that name in our module.  None of these functions is
# looked up in a method table by pysteps - their callers reach them through the module attribute - so the attribute is
# what has to change:
SWAPS = (
    # the member loops call probmatching.nonparam_match_empirical_cdf(...): nowcasts/steps.py:1199, sprog.py:421,
    # sseps.py:783,804, blending/steps.py:3333; calls with ignore_indices and declined inputs go to the stock function
    ("probmatching", "postprocessing.probmatching", ("nonparam_match_empirical_cdf",), "probmatching:"),
    # autoregression.iterate_ar_model(...): nowcasts/steps.py:1095,1137, sprog.py:398, sseps.py:678,749, anvil.py:483
    ("autoregression", "timeseries.autoregression", ("iterate_ar_model",), "autoregression:"),
    # the incremental precipitation mask, nowcast_utils.compute_dilated_mask(...): nowcasts/steps.py:983,1210,
    # sseps.py:472,821
    ("dilated_mask", "nowcasts.utils", ("compute_dilated_mask",), "nowcasts.utils:"),
    # verification.interface.get_method is an if-chain that imports fss from its module when it is called
    # (interface.py:169), and the reference's own fss calls the module's fss_accum
    ("fss", "verification.spatialscores", ("fss", "fss_accum"), "verification:"),
    # get_method imports the two _fct functions from their modules when it is called (interface.py:167-168); the
    # offline scores and declined inputs run the stock functions
    ("detscores", "verification.detcatscores", ("det_cat_fct", "det_cat_fct_accum"), "verification:"),
    ("detscores", "verification.detcontscores", ("det_cont_fct", "det_cont_fct_accum"), "verification:"),
    # get_method imports CRPS, reldiag and ROC_curve from the module when it is called (interface.py:239); the _init
    # and _compute functions stay the reference's: objects of either side are interchangeable
    ("probscores", "verification.probscores", "SWAPPED", "verification:"),
    # get_method(..., type="ensemble") imports ensemble_skill and ensemble_spread from the module when it is called
    # (interface.py:227); rankhist stays the reference's (its ties are broken at random)
    ("ensscores", "verification.ensscores", ("ensemble_skill", "ensemble_spread"), "verification:"),
    # nowcasts.steps(noise_stddev_adj="auto") looks noise.utils.compute_noise_stddev_adjs up when it is called
    # (nowcasts/steps.py:760)
    ("noise_stddev_adj", "noise.utils", ("compute_noise_stddev_adjs",), "noise.utils:"),
    # utils.interface.get_method("rapsd") builds its table from spectral.rapsd when it is called, and
    # noise.fftgenerators.initialize_param_2d_fft_filter calls utils.spectral.rapsd (fftgenerators.py:150).  The
    # reference's downscaling.rainfarm binds the name when it is imported, uses it for spectral fusion alone and keeps
    # the stock function; the device RainFARM hands spectral fusion to the reference and needs no rapsd
    ("rapsd", "utils.spectral", ("rapsd",), "utils.spectral:"),
    # correlation.temporal_autocorrelation(...) per cascade level in front of the main loops: nowcasts/steps.py:840,
    # sprog.py:290, sseps.py:445, blending/steps.py:1491, pca_ens_kalman_filter.py:445, and anvil.py's moving-window
    # form; the multivariate function stays the reference's
    ("correlation", "timeseries.correlation", ("temporal_autocorrelation",), "correlation:"),
)


def swap(mod, name, ours):
    """Put ``ours`` in place of ``mod.<name>`` and park the stock function as ``mod._reference_<name>``."""
    if not hasattr(mod, "_reference_" + name):
        setattr(mod, "_reference_" + name, getattr(mod, name))
    setattr(mod, name, ours)


def restore(mod, name):
    """Undo :func:`swap`; harmless when nothing is parked."""
    stock = getattr(mod, "_reference_" + name, None)
    if stock is not None:
        setattr(mod, name, stock)
        delattr(mod, "_reference_" + name)


def _rows(key):
    for row_key, module, names, prefix in SWAPS:
        if row_key == key:
            ref_mod = importlib.import_module("pysteps." + module)
            hip_mod = importlib.import_module(__package__ + "." + module)
            yield ref_mod, hip_mod, getattr(hip_mod, names) if isinstance(names, str) else names, prefix


def patch(key):
    """Swap the functions of ``key`` into pysteps' modules.  Returns the labels of what was swapped: none for a module
    whose functions are in place already."""
    added = []
    for ref_mod, hip_mod, names, prefix in _rows(key):
        if getattr(ref_mod, names[-1]) is getattr(hip_mod, names[-1]):
            continue
        for name in names:
            swap(ref_mod, name, getattr(hip_mod, name))
            added.append(prefix + name)
    return added


def unpatch(key):
    """Undo :func:`patch`; harmless when nothing is patched."""
    for ref_mod, _, names, _ in _rows(key):
        for name in names:
            restore(ref_mod, name)
