"""Plug the HIP operators into pysteps' own method tables.

pysteps looks the two hot-path operators up by name in module-level dicts
(pysteps/motion/interface.py:36-46 ``_methods``;
pysteps/extrapolation/interface.py:107-111 ``_extrapolation_methods``); there is
no entry-point discovery for them.  ``register()`` inserts the HIP callables under
new names, so that every caller that takes a method *name* - ``nowcasts.extrapolation``,
``nowcasts.steps`` (``extrap_method=``), sprog/anvil/linda/sseps, the blending
module, user scripts calling ``motion.get_method("LK_hip")`` - picks them up
unchanged.  With ``override=True`` the stock names ("semilagrangian", "lk",
"lucaskanade") are replaced as well (the reference's own identity tests
pysteps/tests/test_interfaces.py:69-78,220-233 then fail by design).
"""

from ._reference import patch, restore, swap, unpatch

FFT_NAME = "hip"
CASCADE_NAME = "fft_hip"  # pysteps.cascade.get_method("fft_hip") -> (decomposition_fft, recompose_fft)
NOISE_NAMES = {"parametric_hip": "parametric", "nonparametric_hip": "nonparametric"}
# noise_method names whose initialiser AND generator are the device's (noise/ssft.py): name -> initialiser
SSFT_NAMES = {"ssft_hip": "initialize_nonparam_2d_ssft_filter", "nested_hip": "initialize_nonparam_2d_nested_filter"}
BPS_NAME = "bps_hip"  # vel_pert_method: the reference's generate_bps behind an initialiser that shares the unit fields
EXTRAPOLATION_NAMES = ("semilagrangian_hip",)
MOTION_NAMES = ("lk_hip", "lucaskanade_hip")
DARTS_NAME = "darts_hip"  # the stock "darts" stays the reference's, with or without override
PROESMANS_NAME = "proesmans_hip"  # likewise the stock "proesmans"
FEATURE_NAMES = {"blob_hip": "blob", "shitomasi_hip": "shitomasi"}  # pysteps.feature.get_method(...)
POSTPROCESSING_NAMES = {"mean": "mean", "excprob": "excprob"}  # pysteps.postprocessing.get_method(name + "_hip", "ensemblestats")
BLENDING_NAMES = ("linear_blending_hip", "salient_blending_hip")  # the stock names stay the reference's
_STOCK_EXTRAPOLATION =("semilagrangian",)
_STOCK_MOTION = ("lk", "lucaskanade")


def register_into(motion_methods, extrapolation_methods, override=False):
    """Insert the callables into the given dicts (either may be None). Returns the names added."""
    from .extrapolation.semilagrangian import extrapolate
    from .motion.darts import DARTS
    from .motion.lucaskanade import dense_lucaskanade
    from .motion.proesmans import proesmans

    added = []
    if extrapolation_methods is not None:
        for name in EXTRAPOLATION_NAMES + (_STOCK_EXTRAPOLATION if override else ()):
            extrapolation_methods[name] = extrapolate
            added.append("extrapolation:" + name)
    if motion_methods is not None:
        for name in MOTION_NAMES + (_STOCK_MOTION if override else ()):
            motion_methods[name] = dense_lucaskanade
            added.append("motion:" + name)
        motion_methods[DARTS_NAME] = DARTS
        added.append("motion:" + DARTS_NAME)
        motion_methods[PROESMANS_NAME] = proesmans
        added.append("motion:" + PROESMANS_NAME)
    return added


# pysteps modules that bind the generic nowcast loop by name (``from pysteps.nowcasts.utils import
# nowcast_main_loop``): steps.py:26, sprog.py, anvil.py, linda.py
_MAIN_LOOP_USERS = ("steps", "sprog", "anvil", "linda")


def _main_loop_users():
    """``(name, module)`` of the nowcast modules that import and bind the loop."""
    import importlib  # noqa: PLC0415

    for name in _MAIN_LOOP_USERS:
        try:
            mod = importlib.import_module("pysteps.nowcasts." + name)
        except Exception:
            continue  # optional dependencies of that nowcast module are missing
        if hasattr(mod, "nowcast_main_loop"):
            yield name, mod


def _hip_aware_get_method(reference_get_method):
    """pysteps.utils.interface.get_method hard-codes the FFT method names (interface.py:240-243: an
    ``if name in ["numpy", "pyfftw", "scipy"]`` in front of the method dict), so a new FFT method
    cannot be added to a table: the lookup function itself is wrapped - ``"hip"`` is answered here,
    everything else goes to the reference function unchanged."""
    import functools  # noqa: PLC0415

    @functools.wraps(reference_get_method)
    def get_method(name="", **kwargs):
        if isinstance(name, str) and name.lower() == FFT_NAME:
            if "shape" not in kwargs:
                raise KeyError("mandatory keyword argument shape not given")  # interface.py:241-242
            from .utils.fft import get_hip  # noqa: PLC0415

            kwargs = dict(kwargs)
            return get_hip(kwargs.pop("shape"), **kwargs)
        return reference_get_method(name, **kwargs)

    get_method._pysteps_amd_reference = reference_get_method
    return get_method


def register_fft():
    """Make ``fft_method="hip"`` resolve (``pysteps.utils.get_method("hip", shape=...)``): the
    callers that take an FFT method name - nowcasts.steps / sseps / linda, the noise generators,
    the cascade decomposition - then run their transforms through csrc/fft.hip."""
    import pysteps.utils as utils_pkg  # noqa: PLC0415
    import pysteps.utils.interface as utils_if  # noqa: PLC0415

    if hasattr(utils_if.get_method, "_pysteps_amd_reference"):
        return []
    wrapped = _hip_aware_get_method(utils_if.get_method)
    utils_if.get_method = wrapped
    utils_pkg.get_method = wrapped
    try:  # the one module that binds the function by name (blending/utils.py:30)
        import pysteps.blending.utils as blending_utils  # noqa: PLC0415

        if hasattr(blending_utils, "utils_get_method"):
            blending_utils.utils_get_method = wrapped
    except Exception:
        pass
    return ["fft:" + FFT_NAME]


def register_spectral():
    """Insert the device cascade decomposition and noise generator into the reference's method tables
    (pysteps/cascade/interface.py:15-18 ``_cascade_methods``, pysteps/noise/interface.py:24-45
    ``_noise_methods``): ``decomp_method="fft_hip"`` and ``noise_method="nonparametric_hip"`` /
    ``"parametric_hip"`` (the reference's filter initialisation paired with the HIP generator), and
    ``noise_method="ssft_hip"`` / ``"nested_hip"`` (the device's local-filter initialisers with its composite
    generator)."""
    import pysteps.cascade.interface as cas_if  # noqa: PLC0415
    import pysteps.noise.interface as noise_if  # noqa: PLC0415

    from .cascade.decomposition import decomposition_fft, recompose_fft  # noqa: PLC0415
    from .noise.fftgenerators import generate_noise_2d_fft_filter  # noqa: PLC0415

    added = []
    cas_if._cascade_methods[CASCADE_NAME] = (decomposition_fft, recompose_fft)
    added.append("cascade:" + CASCADE_NAME)
    for name, stock in NOISE_NAMES.items():
        init = noise_if._noise_methods[stock][0]
        noise_if._noise_methods[name] = (init, generate_noise_2d_fft_filter)
        added.append("noise:" + name)
    from .noise import ssft  # noqa: PLC0415

    for name, init in SSFT_NAMES.items():  # the stock "ssft" / "nested" stay the reference's
        noise_if._noise_methods[name] = (getattr(ssft, init), ssft.generate_noise_2d_ssft_filter)
        added.append("noise:" + name)
    from .noise.motion import initialize_bps  # noqa: PLC0415

    noise_if._noise_methods[BPS_NAME] = (initialize_bps, noise_if._noise_methods["bps"][1])
    added.append("noise:" + BPS_NAME)
    return added


def register_features(override=False):
    """Insert the HIP feature detectors into the reference's table (pysteps/feature/interface.py:26-29
    ``_detection_methods``) as ``"blob_hip"`` / ``"shitomasi_hip"`` (and under the stock names with ``override``):
    ``pysteps.feature.get_method("blob_hip")``, and through it ``dense_lucaskanade(fd_method="blob_hip")`` of the
    REFERENCE's Lucas-Kanade routine, then run the scale-space / corner kernels.  (``pysteps_amd``'s own
    ``dense_lucaskanade`` takes ``fd_method="blob"`` / ``"shitomasi"`` directly.)"""
    import pysteps.feature.interface as feat_if  # noqa: PLC0415

    from .feature import blob, shitomasi  # noqa: PLC0415

    added = []
    for name, stock in FEATURE_NAMES.items():
        fn = blob.detection if stock == "blob" else shitomasi.detection
        for key in (name,) + ((stock,) if override else ()):
            feat_if._detection_methods[key] = fn
            added.append("feature:" + key)
    return added


def unregister_fft():
    import pysteps.utils as utils_pkg  # noqa: PLC0415
    import pysteps.utils.interface as utils_if  # noqa: PLC0415

    ref = getattr(utils_if.get_method, "_pysteps_amd_reference", None)
    if ref is not None:
        utils_if.get_method = ref
        utils_pkg.get_method = ref


# The swaps of module attributes.  ``_reference.SWAPS`` lists, per key, the functions that change and why it is the
# attribute - no method table - that has to change; the stock function stays reachable as ``_reference_<name>`` on the
# reference's module, and inputs the device path declines are handed to it.


def patch_probmatching():
    """Replace ``pysteps.postprocessing.probmatching.nonparam_match_empirical_cdf`` by the device version."""
    return patch("probmatching")


def unpatch_probmatching():
    """Undo :func:`patch_probmatching`."""
    unpatch("probmatching")


def patch_autoregression():
    """Replace ``pysteps.timeseries.autoregression.iterate_ar_model`` by the device version."""
    return patch("autoregression")


def unpatch_autoregression():
    """Undo :func:`patch_autoregression`."""
    unpatch("autoregression")


def patch_dilated_mask():
    """Replace ``pysteps.nowcasts.utils.compute_dilated_mask`` by the device version."""
    return patch("dilated_mask")


def unpatch_dilated_mask():
    """Undo :func:`patch_dilated_mask`."""
    unpatch("dilated_mask")


def patch_fss():
    """Replace ``fss`` and ``fss_accum`` of ``pysteps.verification.spatialscores`` by the device versions
    (:mod:`pysteps_amd.verification.spatialscores`): ``get_method("fss")`` and the reference's own ``fss`` then count on
    the device."""
    return patch("fss")


def unpatch_fss():
    """Undo :func:`patch_fss`."""
    unpatch("fss")


def patch_detscores():
    """Replace ``det_cat_fct`` and ``det_cat_fct_accum`` of ``pysteps.verification.detcatscores`` and ``det_cont_fct`` and
    ``det_cont_fct_accum`` of ``pysteps.verification.detcontscores`` by the device versions
    (:mod:`pysteps_amd.verification.detcatscores`, :mod:`pysteps_amd.verification.detcontscores`)."""
    return patch("detscores")


def unpatch_detscores():
    """Undo :func:`patch_detscores`."""
    unpatch("detscores")


def patch_probscores():
    """Replace ``CRPS``, ``reldiag`` and ``ROC_curve`` and their ``_accum`` functions in
    ``pysteps.verification.probscores`` by the device versions (:mod:`pysteps_amd.verification.probscores`)."""
    return patch("probscores")


def unpatch_probscores():
    """Undo :func:`patch_probscores`."""
    unpatch("probscores")


def patch_ensscores():
    """Replace ``ensemble_skill`` and ``ensemble_spread`` of ``pysteps.verification.ensscores`` by the device versions
    (:mod:`pysteps_amd.verification.ensscores`); ``rankhist`` stays the reference's."""
    return patch("ensscores")


def unpatch_ensscores():
    """Undo :func:`patch_ensscores`."""
    unpatch("ensscores")


def patch_noise_stddev_adj():
    """Replace ``pysteps.noise.utils.compute_noise_stddev_adjs`` by the device version
    (:mod:`pysteps_amd.noise.utils`); calls the device path declines run the reference's function with a
    ``RuntimeWarning``."""
    return patch("noise_stddev_adj")


def unpatch_noise_stddev_adj():
    """Undo :func:`patch_noise_stddev_adj`."""
    unpatch("noise_stddev_adj")


def patch_rapsd():
    """Replace ``pysteps.utils.spectral.rapsd`` by the device version (:mod:`pysteps_amd.utils.spectral`); inputs the
    device path declines run the reference's function with a ``RuntimeWarning``."""
    return patch("rapsd")


def unpatch_rapsd():
    """Undo :func:`patch_rapsd`."""
    unpatch("rapsd")


def patch_correlation():
    """Replace ``pysteps.timeseries.correlation.temporal_autocorrelation`` by the device version
    (:mod:`pysteps_amd.timeseries.correlation`): the nowcast modules reach it through the module attribute, so steps,
    sprog, sseps, blending.steps, pca_ens_kalman_filter and anvil then estimate their AR models from device sums;
    inputs the device path declines run the reference's function with a ``RuntimeWarning``."""
    return patch("correlation")


def unpatch_correlation():
    """Undo :func:`patch_correlation`."""
    unpatch("correlation")


def register_nowcasts():
    """Add ``"anvil_hip"`` (:func:`pysteps_amd.nowcasts.anvil.forecast`) and ``"lagrangian_probability_hip"``
    (:func:`pysteps_amd.nowcasts.lagrangian_probability.forecast`) to pysteps' nowcast table
    (pysteps/nowcasts/interface.py ``_nowcast_methods``); the stock ``"anvil"`` and ``"lagrangian_probability"`` stay
    the reference's."""
    import pysteps.nowcasts.interface as now_if  # noqa: PLC0415

    from .nowcasts.anvil import forecast  # noqa: PLC0415
    from .nowcasts.lagrangian_probability import forecast as lagprob_forecast  # noqa: PLC0415

    now_if._nowcast_methods["anvil_hip"] = forecast
    now_if._nowcast_methods["lagrangian_probability_hip"] = lagprob_forecast
    return ["nowcast:anvil_hip", "nowcast:lagrangian_probability_hip"]


def register_downscaling():
    """Add ``"rainfarm_hip"`` (:func:`pysteps_amd.downscaling.rainfarm.downscale`) to pysteps' downscaling table
    (pysteps/downscaling/interface.py ``_downscale_methods``); the stock ``"rainfarm"`` stays the reference's."""
    import pysteps.downscaling.interface as ds_if  # noqa: PLC0415

    from .downscaling.rainfarm import downscale  # noqa: PLC0415

    ds_if._downscale_methods["rainfarm_hip"] = downscale
    return ["downscaling:rainfarm_hip"]


def register_blending():
    """Add ``"linear_blending_hip"`` and ``"salient_blending_hip"`` (:func:`pysteps_amd.blending.linear_blending.forecast`,
    the latter with ``saliency=True``) to pysteps' blending table (pysteps/blending/interface.py
    ``_blending_methods``); the stock ``"linear_blending"`` and ``"salient_blending"`` stay the reference's."""
    import pysteps.blending.interface as blend_if  # noqa: PLC0415

    from .blending.interface import get_method  # noqa: PLC0415

    added = []
    for name in BLENDING_NAMES:
        blend_if._blending_methods[name] = get_method(name)
        added.append("blending:" + name)
    return added


def register_postprocessing(override=False):
    """Add ``"mean_hip"`` and ``"excprob_hip"`` (:mod:`pysteps_amd.postprocessing.ensemblestats`) to pysteps' ensemble
    statistics table (pysteps/postprocessing/interface.py ``_ensemblestats_methods``:
    ``pysteps.postprocessing.get_method("excprob_hip", "ensemblestats")``); the stock ``"mean"`` and ``"excprob"`` are
    only replaced with ``override``.  ``"banddepth"`` stays the reference's (its ties are broken at random)."""
    import pysteps.postprocessing.interface as post_if  # noqa: PLC0415

    from .postprocessing import ensemblestats  # noqa: PLC0415

    added = []
    for name, fn in POSTPROCESSING_NAMES.items():
        for key in (name + "_hip",) + ((name,) if override else ()):
            post_if._ensemblestats_methods[key] = getattr(ensemblestats, fn)
            added.append("ensemblestats:" + key)
    return added


def register(override=False, patch_main_loop=False, fft=True, probmatching=False, autoregression=False,
             dilated_mask=False, fss=False, noise_stddev_adj=False, detscores=False, rapsd=False, probscores=False,
             ensscores=False, correlation=False):
    """Register with an importable pysteps; raises ImportError if pysteps is absent.

    ``patch_main_loop=True`` also installs the device-resident generic nowcast loop
    (:func:`pysteps_amd.nowcasts.utils.nowcast_main_loop`) in the nowcast modules: with
    ``extrap_method="semilagrangian_hip"`` all ensemble members are then advected by one kernel
    launch per time step and their trajectories stay in HBM; any other extrapolator runs exactly as
    before.  With that loop ``nowcasts.steps`` also runs its member update on device-resident state
    (:mod:`pysteps_amd.nowcasts.steps_resident`).  Parity level of that update: the default keeps the AR
    history as spectra and reproduces the reference's fields up to rounding, not bit for bit (identical NaN
    masks, no pixel decided differently by a threshold or a rank in the tests, 8e-8 relative L2 end to end);
    ``PYSTEPS_HIP_RESIDENT_DOMAIN=spatial`` selects the chain of spatial operators whose element-wise steps
    are bit-identical with the reference's.  :func:`unpatch_main_loop` restores the reference loop.

    ``fss=True`` makes ``pysteps.verification`` count the fractions skill score on the device (:func:`patch_fss`;
    :func:`unpatch_fss` undoes it).  ``noise_stddev_adj=True`` makes ``nowcasts.steps(noise_stddev_adj="auto")``
    compute its adjustment coefficients on the device (:func:`patch_noise_stddev_adj`;
    :func:`unpatch_noise_stddev_adj` undoes it).  ``detscores=True`` makes ``pysteps.verification`` count contingency
    tables and sum the continuous error moments on the device (:func:`patch_detscores`; :func:`unpatch_detscores`
    undoes it).  ``rapsd=True`` makes ``pysteps.utils.spectral.rapsd`` bin its spectra on the device
    (:func:`patch_rapsd`; :func:`unpatch_rapsd` undoes it).  ``probscores=True`` makes
    ``pysteps.verification.probscores`` accumulate the CRPS, reliability diagrams and ROC curves on the device
    (:func:`patch_probscores`; :func:`unpatch_probscores` undoes it).  ``ensscores=True`` makes
    ``pysteps.verification.ensscores`` compute ensemble skill and spread on the device (:func:`patch_ensscores`;
    :func:`unpatch_ensscores` undoes it).  ``correlation=True`` makes
    ``pysteps.timeseries.correlation.temporal_autocorrelation`` take its sums on the device (:func:`patch_correlation`;
    :func:`unpatch_correlation` undoes it).

    ``"rainfarm_hip"`` joins ``pysteps.downscaling``'s method table (:func:`register_downscaling`), and
    ``"linear_blending_hip"`` and ``"salient_blending_hip"`` join ``pysteps.blending``'s (:func:`register_blending`)."""
    import pysteps.extrapolation.interface as ext_if  # noqa: PLC0415
    import pysteps.motion.interface as mot_if  # noqa: PLC0415

    added = register_into(mot_if._methods, ext_if._extrapolation_methods, override=override)
    try:
        added += register_features(override=override)
    except ImportError:
        pass  # pysteps.feature needs none of its optional dependencies at import time; a stripped-down install may lack it
    try:
        added += register_nowcasts()
    except ImportError:
        pass  # pysteps.nowcasts imports every nowcast module; a stripped-down install may lack one's dependencies
    try:
        added += register_postprocessing(override=override)
    except ImportError:
        pass  # pysteps.postprocessing imports its diagnostics' optional dependencies lazily; a stripped-down install may lack it
    try:
        added += register_downscaling()
    except ImportError:
        pass  # an older or stripped-down install may lack pysteps.downscaling
    try:
        added += register_blending()
    except ImportError:
        pass  # pysteps.blending imports every blending module; a stripped-down install may lack one's dependencies
    if fft:
        added += register_fft()
        added += register_spectral()
    for key, wanted in (("probmatching", probmatching), ("autoregression", autoregression), ("dilated_mask", dilated_mask),
                        ("fss", fss), ("noise_stddev_adj", noise_stddev_adj), ("detscores", detscores), ("rapsd", rapsd),
                        ("probscores", probscores), ("ensscores", ensscores), ("correlation", correlation)):
        if wanted:
            added += patch(key)
    if patch_main_loop:
        from .nowcasts.utils import nowcast_main_loop  # noqa: PLC0415

        for name, mod in _main_loop_users():
            swap(mod, "nowcast_main_loop", nowcast_main_loop)
            added.append("main_loop:" + name)
    return added


def unpatch_main_loop():
    """Undo ``register(patch_main_loop=True)``."""
    for _, mod in _main_loop_users():
        restore(mod, "nowcast_main_loop")
