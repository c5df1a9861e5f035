"""The fallback contract of the operators that ``register`` can swap into pysteps' module attributes, through public
functions and ``<reference module>._reference_<name>`` alone: what ``patch_*`` returns, where the stock function is
parked, that a declined input reaches it, and that ``unpatch_*`` leaves nothing behind.  One declined host input per
key, chosen among those whose decision is taken before any device call.  Without pysteps a declined input raises; the
types and texts are recorded here."""

import contextlib
import importlib
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import ROOT


def _warns(ours, category, match):
    """Our function warns when it hands the input over; the stock function, called directly, has nothing to say."""
    return pytest.warns(category, match=match) if ours else contextlib.nullcontext()


def _fields(dtype=np.int64):
    rng = np.random.default_rng(3)
    return rng.integers(0, 5, (12, 10)).astype(dtype), rng.integers(0, 5, (12, 10)).astype(dtype)


def _probmatching(fn, ours):
    rng = np.random.default_rng(0)  # below the size a host array is uploaded at
    return fn(rng.random((9, 7)), rng.random((9, 7)))


def _autoregression(fn, ours):
    rng = np.random.default_rng(1)  # a small host series stays with NumPy
    return fn(rng.random((2, 8, 8)), [0.5, 0.3, 0.6], eps=rng.random((8, 8)))


def _dilated_mask(fn, ours):
    rng = np.random.default_rng(2)  # a small host mask
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    return fn(rng.random((40, 50)) < 0.1, cross, 3)


def _fss_accum(fn, ours):
    X_f, X_o = _fields()
    obj = dict(thr=1, scale=3, sum_fct_sq=0.0, sum_fct_obs=0.0, sum_obs_sq=0.0)
    with _warns(ours, UserWarning, match="pysteps_amd fss_accum: dtype int64 - running the reference's function"):
        fn(obj, X_f, X_o)
    return [obj["sum_fct_sq"], obj["sum_fct_obs"], obj["sum_obs_sq"]]


def _fss(fn, ours):
    X_f, X_o = _fields()
    with _warns(ours, UserWarning, match="pysteps_amd fss_accum: dtype int64 - running the reference's function"):
        return fn(X_f, X_o, 1, 3)


def _det_cat_fct_accum(fn, ours):
    from pysteps.verification.detcatscores import det_cat_fct_init

    pred, obs = _fields()
    contab = det_cat_fct_init(1)
    with _warns(ours, RuntimeWarning, match="pysteps_amd det_cat_fct_accum: dtype int64 - running the reference's function"):
        fn(contab, pred, obs)
    return [contab[k] for k in ("hits", "misses", "false_alarms", "correct_negatives")]


def _det_cat_fct(fn, ours):
    pred, obs = _fields()
    with _warns(ours, RuntimeWarning, match="pysteps_amd det_cat_fct_accum: dtype int64 - running the reference's function"):
        got = fn(pred, obs, 1, scores=["POD", "FAR"])
    return [got["POD"], got["FAR"]]


def _det_cont_fct_accum(fn, ours):
    from pysteps.verification.detcontscores import det_cont_fct_init

    pred, obs = _fields()
    err = det_cont_fct_init()
    with _warns(ours, RuntimeWarning, match="pysteps_amd det_cont_fct_accum: dtype int64 - running the reference's function"):
        fn(err, pred, obs)
    return [err[k] for k in ("n", "me", "mse", "mae")]


def _det_cont_fct(fn, ours):
    pred, obs = _fields()
    with _warns(ours, RuntimeWarning, match="pysteps_amd det_cont_fct_accum: dtype int64 - running the reference's function"):
        got = fn(pred, obs, scores=["ME", "RMSE"])
    return [got["ME"], got["RMSE"]]


def _ensemble():
    rng = np.random.default_rng(4)
    return rng.integers(0, 5, (4, 12, 10)), rng.integers(0, 5, (12, 10))


def _crps_accum(fn, ours):
    X_f, X_o = _ensemble()
    obj = {"CRPS_sum": 0.0, "n": 0.0}
    with _warns(ours, RuntimeWarning, match="pysteps_amd CRPS_accum: dtype int64 - running the reference's function"):
        fn(obj, X_f, X_o)
    return [obj["CRPS_sum"], obj["n"]]


def _crps(fn, ours):
    X_f, X_o = _ensemble()
    with _warns(ours, RuntimeWarning, match="pysteps_amd CRPS_accum: dtype int64 - running the reference's function"):
        return fn(X_f, X_o)


def _probabilities():
    rng = np.random.default_rng(5)
    return rng.integers(0, 2, (12, 10)), rng.integers(0, 5, (12, 10))  # integer probabilities: declined by dtype


def _reldiag_accum(fn, ours):
    from pysteps.verification.probscores import reldiag_init

    P_f, X_o = _probabilities()
    obj = reldiag_init(1)
    with _warns(ours, RuntimeWarning, match="pysteps_amd reldiag_accum: .* - running the reference's function"):
        fn(obj, P_f, X_o)
    return [obj["X_sum"], obj["Y_sum"], obj["num_idx"], obj["sample_size"]]


def _reldiag(fn, ours):
    P_f, X_o = _probabilities()
    with _warns(ours, RuntimeWarning, match="pysteps_amd reldiag_accum: .* - running the reference's function"):
        return list(fn(P_f, X_o, 1))


def _roc_accum(fn, ours):
    from pysteps.verification.probscores import ROC_curve_init

    P_f, X_o = _probabilities()
    obj = ROC_curve_init(1)
    with _warns(ours, RuntimeWarning, match="pysteps_amd ROC_curve_accum: .* - running the reference's function"):
        fn(obj, P_f, X_o)
    return [obj["hits"], obj["misses"], obj["false_alarms"], obj["corr_neg"]]


def _roc(fn, ours):
    P_f, X_o = _probabilities()
    with _warns(ours, RuntimeWarning, match="pysteps_amd ROC_curve_accum: .* - running the reference's function"):
        return list(fn(P_f, X_o, 1))


def _noise_stddev_adjs(fn, ours):
    from pysteps.cascade.bandpass_filters import filter_gaussian
    from pysteps.cascade.decomposition import decomposition_fft
    from pysteps.noise.fftgenerators import generate_noise_2d_fft_filter, initialize_nonparam_2d_fft_filter

    R = np.random.default_rng(6).gamma(0.4, 4.0, (32, 32)).astype(np.float32)
    F, noise_filter = filter_gaussian(R.shape, 3), initialize_nonparam_2d_fft_filter(R.astype(np.float64))
    with _warns(ours, RuntimeWarning, match="pysteps_amd compute_noise_stddev_adjs: R is float32, .* - running the "
                                            "reference's function"):
        return fn(R, 0.5, 0.1, F, decomposition_fft, noise_filter, generate_noise_2d_fft_filter, 2, seed=11)


def _rapsd(fn, ours):
    field = np.random.default_rng(7).integers(0, 9, (16, 16))
    with _warns(ours, RuntimeWarning, match="pysteps_amd rapsd: a field of dtype int64 - running the reference's function"):
        return fn(field, fft_method=np.fft)


# key -> (the labels patch_<key>() returns, {reference module: {name: a declined call of that function}})
SWAPS = {
    "probmatching": (["probmatching:nonparam_match_empirical_cdf"],
                     {"postprocessing.probmatching": {"nonparam_match_empirical_cdf": _probmatching}}),
    "autoregression": (["autoregression:iterate_ar_model"], {"timeseries.autoregression": {"iterate_ar_model": _autoregression}}),
    "dilated_mask": (["nowcasts.utils:compute_dilated_mask"], {"nowcasts.utils": {"compute_dilated_mask": _dilated_mask}}),
    "fss": (["verification:fss", "verification:fss_accum"],
            {"verification.spatialscores": {"fss": _fss, "fss_accum": _fss_accum}}),
    "detscores": (["verification:det_cat_fct", "verification:det_cat_fct_accum", "verification:det_cont_fct",
                   "verification:det_cont_fct_accum"],
                  {"verification.detcatscores": {"det_cat_fct": _det_cat_fct, "det_cat_fct_accum": _det_cat_fct_accum},
                   "verification.detcontscores": {"det_cont_fct": _det_cont_fct, "det_cont_fct_accum": _det_cont_fct_accum}}),
    "probscores": (["verification:CRPS", "verification:CRPS_accum", "verification:reldiag", "verification:reldiag_accum",
                    "verification:ROC_curve", "verification:ROC_curve_accum"],
                   {"verification.probscores": {"CRPS": _crps, "CRPS_accum": _crps_accum, "reldiag": _reldiag,
                                                "reldiag_accum": _reldiag_accum, "ROC_curve": _roc, "ROC_curve_accum": _roc_accum}}),
    "noise_stddev_adj": (["noise.utils:compute_noise_stddev_adjs"], {"noise.utils": {"compute_noise_stddev_adjs": _noise_stddev_adjs}}),
    "rapsd": (["utils.spectral:rapsd"], {"utils.spectral": {"rapsd": _rapsd}}),
}


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("key", sorted(SWAPS))
def test_patch_parks_the_stock_function_and_unpatch_leaves_nothing(ref_pysteps, key):
    from pysteps_amd import register

    labels, modules = SWAPS[key]
    patch, unpatch = getattr(register, "patch_" + key), getattr(register, "unpatch_" + key)
    sites = [(importlib.import_module("pysteps." + mod), importlib.import_module("pysteps_amd." + mod), name, call)
             for mod, names in modules.items() for name, call in names.items()]
    stock = [getattr(ref_mod, name) for ref_mod, _, name, _ in sites]
    assert labels == [label.split(":")[0] + ":" + name for label, (_, _, name, _) in zip(labels, sites)]
    want = [call(fn, False) for fn, (_, _, _, call) in zip(stock, sites)]
    try:
        for _ in range(2):  # a patch -> unpatch -> patch cycle behaves like the first patch
            assert patch() == labels
            assert patch() == []  # already in place
            for (ref_mod, hip_mod, name, call), fn, expected in zip(sites, stock, want):
                assert getattr(ref_mod, name) is getattr(hip_mod, name) and getattr(hip_mod, name) is not fn
                assert getattr(ref_mod, "_reference_" + name) is fn
                assert _same(call(getattr(ref_mod, name), True), expected), name  # declined: the stock function's answer
            unpatch()
            for (ref_mod, _, name, _), fn in zip(sites, stock):
                assert getattr(ref_mod, name) is fn and not hasattr(ref_mod, "_reference_" + name)
            unpatch()  # harmless when nothing is patched
            for (ref_mod, _, name, _), fn in zip(sites, stock):
                assert getattr(ref_mod, name) is fn and not hasattr(ref_mod, "_reference_" + name)
    finally:
        unpatch()


def test_register_keywords_return_the_labels_of_patch(ref_pysteps):
    from pysteps_amd import register

    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            register.register()  # (the FFT method name is only reported by the call that installs it)
            plain = register.register()
            for key, (labels, _) in SWAPS.items():
                assert register.register(**{key: True}) == plain + labels, key
                assert register.register(**{key: True}) == plain, key
                getattr(register, "unpatch_" + key)()
    finally:
        for key in SWAPS:
            getattr(register, "unpatch_" + key)()
        register.unregister_fft()


def test_main_loop_swap_and_unpatch(ref_pysteps):
    from pysteps.nowcasts.utils import nowcast_main_loop as stock

    from pysteps_amd import register
    from pysteps_amd.nowcasts.utils import nowcast_main_loop

    users = [importlib.import_module("pysteps.nowcasts." + name) for name in ("steps", "sprog", "anvil", "linda")]
    labels = ["main_loop:steps", "main_loop:sprog", "main_loop:anvil", "main_loop:linda"]
    assert all(mod.nowcast_main_loop is stock for mod in users)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            register.register()
            plain = register.register()
            for _ in range(2):
                assert register.register(patch_main_loop=True) == plain + labels
                assert all(mod.nowcast_main_loop is nowcast_main_loop for mod in users)
                assert all(mod._reference_nowcast_main_loop is stock for mod in users)
                register.register(patch_main_loop=True)  # a second swap keeps the stock loop parked
                assert all(mod._reference_nowcast_main_loop is stock for mod in users)
                register.unpatch_main_loop()
                assert all(mod.nowcast_main_loop is stock and not hasattr(mod, "_reference_nowcast_main_loop") for mod in users)
                register.unpatch_main_loop()  # harmless when nothing is patched
                assert all(mod.nowcast_main_loop is stock for mod in users)
    finally:
        register.unpatch_main_loop()
        register.unregister_fft()


# without pysteps a declined host input raises: one operator of each kind of lookup (a plain one, one that register can
# swap in, one that cannot work without the reference's function and lets the ImportError through)
WITHOUT_PYSTEPS = {
    "fftgenerators": ("NotImplementedError",
                      "pysteps_amd generate_noise_2d_fft_filter: spatial domain, half-spectrum filters and power-of-two grids "
                      "run on the HIP path; pysteps is not importable for the rest"),
    "fss_accum": ("NotImplementedError", "pysteps_amd fss_accum: dtype int64 is not implemented on the device and pysteps is not "
                                         "importable"),
    "iterate_ar_model": ("ImportError", "pysteps is blocked in this test"),
}


def test_declined_inputs_raise_without_pysteps():
    code = (
        "import sys\n"
        "class Block:\n"
        "    def find_spec(self, name, path=None, target=None):\n"
        "        if name == 'pysteps' or name.startswith('pysteps.'):\n"
        "            raise ImportError('pysteps is blocked in this test')\n"
        "sys.meta_path.insert(0, Block())\n"
        "import numpy as np\n"
        "from pysteps_amd.noise.fftgenerators import generate_noise_2d_fft_filter\n"
        "from pysteps_amd.timeseries.autoregression import iterate_ar_model\n"
        "from pysteps_amd.verification.spatialscores import fss_accum, fss_init\n"
        "F = {'input_shape': (8, 8), 'use_full_fft': False, 'field': np.ones((8, 5))}\n"
        "calls = {\n"
        "    'fftgenerators': lambda: generate_noise_2d_fft_filter(F, domain='spectral'),\n"
        "    'fss_accum': lambda: fss_accum(fss_init(1, 3), np.ones((6, 5), dtype=np.int64), np.ones((6, 5), dtype=np.int64)),\n"
        "    'iterate_ar_model': lambda: iterate_ar_model(np.zeros((2, 4, 4)), [0.5, 0.1, 0.8]),\n"
        "}\n"
        "for name, call in calls.items():\n"
        "    try:\n"
        "        call()\n"
        "    except Exception as exc:\n"
        "        print('%s|%s|%s' % (name, type(exc).__name__, exc))\n"
        "    else:\n"
        "        print('%s|returned|' % name)\n"
        "assert not any(k == 'pysteps' or k.startswith('pysteps.') for k in sys.modules)\n"
    )
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    got = {line.split("|")[0]: tuple(line.split("|")[1:]) for line in res.stdout.strip().splitlines()}
    assert got == WITHOUT_PYSTEPS


def test_pysteps_is_imported_in_one_place_only():
    """``_reference.py`` finds the reference's functions, ``register.py`` and the ``get_method`` mirrors reach its method
    tables; nothing else imports pysteps, and no module keeps a lookup function of its own."""
    import re

    package = os.path.join(ROOT, "pysteps_amd")
    importers, lookups = [], []
    for folder, _, files in os.walk(package):
        for name in files:
            if not name.endswith(".py"):
                continue
            path = os.path.relpath(os.path.join(folder, name), package)
            source = open(os.path.join(folder, name)).read()
            if re.search(r"^\s*(from|import) pysteps\b", source, re.MULTILINE):
                importers.append(path)
            lookups += [path + ":" + fn for fn in re.findall(r"^\s*def (_reference\w*)", source, re.MULTILINE)]
    allowed = {"_reference.py", "register.py"}
    assert [p for p in importers if p not in allowed and os.path.basename(p) != "interface.py"] == []
    assert lookups == []
