"""Ensemble mean and exceedance probabilities on the device (``pysteps_amd.postprocessing.ensemblestats``,
csrc/ensstats.hip).

Held against tests/golden/ensstats_reference.npz (the unmodified reference's outputs, written by
tools/make_golden_ensstats.py), against the real reference from oracle/_ref at size, and end to end inside the real
``pysteps.nowcasts.steps``.  Every operation of the kernel is an exactly specified IEEE operation in the reference's
order, so every comparison is bit for bit - values, NaN positions and dtype - with no tolerance.
"""

import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import ensstats as restated

pytestmark = pytest.mark.gpu

PATH = os.path.join(GOLDEN, "ensstats_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def case_names():
    return [str(c) for c in np.load(PATH)["cases"]]


def same_bits(got, want):
    """Equal as bit patterns apart from the NaN payload: same dtype, shape and NaN mask, same bits elsewhere."""
    if not isinstance(got, np.ndarray) or got.dtype != want.dtype or got.shape != want.shape:
        return False
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    bits = np.uint64 if want.dtype == np.float64 else np.uint32
    return np.array_equal(got[ok].view(bits), want[ok].view(bits))


@pytest.mark.parametrize("resident", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", case_names())
def test_goldens_bit_identical(golden, name, dtype, resident):
    """mean, excprob and products on every golden case: NumPy in -> NumPy out, DeviceArray in -> DeviceArray out."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.postprocessing import ensemblestats

    X = golden[name + "__X"].astype(dtype)
    arg = DeviceArray.from_host(X) if resident else X
    kind = DeviceArray if resident else np.ndarray

    def host(a):
        assert isinstance(a, kind)
        return a.to_host() if resident else a

    ops = json.loads(str(golden[name + "__ops"]))
    wants = [golden["%s__%s__%d" % (name, dtype, i)] for i in range(len(ops))]
    for op, want in zip(ops, wants):
        got = host(getattr(ensemblestats, op["fn"])(arg, **op["kwargs"]))
        assert same_bits(got, want), op
    # the fused form: every mean variant with every threshold set
    for mop, mwant in zip(ops, wants):
        if mop["fn"] != "mean":
            continue
        for pop, pwant in zip(ops, wants):
            if pop["fn"] != "excprob":
                continue
            m, p = ensemblestats.products(arg, pop["kwargs"]["X_thr"], ignore_nan=pop["kwargs"]["ignore_nan"],
                                          mean_ignore_nan=mop["kwargs"].get("ignore_nan", False),
                                          mean_thr=mop["kwargs"].get("X_thr"))
            assert same_bits(host(m), mwant) and same_bits(host(p), pwant), (mop, pop)
    m, p = ensemblestats.products(arg, [2.5], mean=False)
    assert m is None and same_bits(host(p), restated.excprob(X, [2.5]))
    if not resident:
        assert np.array_equal(X, golden[name + "__X"].astype(dtype), equal_nan=True)  # the input is not modified


def test_two_dimensional_mean_and_trailing_dimensions(golden):
    from pysteps_amd.postprocessing import ensemblestats

    X = golden["k7_53x75__X"]
    assert same_bits(ensemblestats.mean(X[0]), restated.mean(X[0]))  # the field itself, a -0.0 as +0.0 like np.mean
    X5 = np.ascontiguousarray(X[:6, :50, :70].reshape(6, 5, 10, 70))
    got = ensemblestats.excprob(X5, [0.7, 2.5], ignore_nan=True)
    assert got.shape == (2, 5, 10, 70) and same_bits(got, restated.excprob(X5, [0.7, 2.5], ignore_nan=True))
    # a numpy.float64 threshold meets a float32 stack as float64, a Python float as float32
    a = ensemblestats.excprob(X, np.float64(0.7))
    b = ensemblestats.excprob(X, 0.7)
    assert same_bits(a, restated.excprob(X, np.float64(0.7))) and same_bits(b, restated.excprob(X, 0.7))
    assert not np.array_equal(a, b, equal_nan=True)


def synthetic(k, m, n, seed, dtype):
    rng = np.random.default_rng(seed)
    base = rng.gamma(0.6, 4.0, size=(m, n)).astype(np.float32)
    X = np.empty((k, m, n), dtype=dtype)
    for j in range(k):
        f = base * rng.lognormal(0.0, 0.5, size=(m, n)).astype(np.float32)
        f[rng.random((m, n)) < 0.5] = 0.0
        X[j] = f
    X[:, :3] = np.nan
    X[rng.random(X.shape) < 0.001] = np.nan
    X[rng.random(X.shape) < 0.0005] = np.inf
    X[rng.random(X.shape) < 0.0005] = -np.inf
    X[rng.random(X.shape) < 0.01] = 2.5
    X[:, m // 2, n // 2] = np.nan
    return X


@pytest.mark.parametrize("shape,dtype", [((20, 1024, 1024), "float32"), ((7, 640, 710), "float64"), ((5, 1226, 761), "float32")])
def test_real_reference_at_size(ref_pysteps, shape, dtype):
    """The real reference from oracle/_ref on large stacks (the last shape's planes are not 16-byte aligned)."""
    from pysteps.postprocessing import ensemblestats as ref

    from pysteps_amd.device import DeviceArray
    from pysteps_amd.postprocessing import ensemblestats

    X = synthetic(*shape, seed=sum(shape), dtype=dtype)
    thresholds = [0.1, 1.0, 2.5]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        want_mean, want_nanmean = ref.mean(X), ref.mean(X, ignore_nan=True, X_thr=0.1)
        want_p, want_pn = ref.excprob(X, thresholds), ref.excprob(X, thresholds, ignore_nan=True)
    dev = DeviceArray.from_host(X)
    m, p = ensemblestats.products(dev, thresholds)
    assert same_bits(m.to_host(), want_mean) and same_bits(p.to_host(), want_p)
    m, p = ensemblestats.products(dev, thresholds, ignore_nan=True, mean_ignore_nan=True, mean_thr=0.1)
    assert same_bits(m.to_host(), want_nanmean) and same_bits(p.to_host(), want_pn)
    assert same_bits(ensemblestats.mean(X), want_mean) and same_bits(ensemblestats.excprob(X, thresholds), want_p)
    finite = want_p[np.isfinite(want_p)]
    assert np.unique(finite).size >= min(shape[0], 5) and 0.01 < finite.mean() < 0.9  # the case is not trivial


@pytest.mark.parametrize("keep", ["host", "device"])
def test_accumulator_equals_products_per_lead_time(golden, keep):
    """float32 device members are accumulated as float64: the products of the widened members, which is what the
    reference computes from a nowcast's float64 block."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.postprocessing import ensemblestats

    X = golden["k20_48x84__X"]
    leads = [X, X[::-1].copy(), np.roll(X, 3, axis=2)]
    thresholds = [0.5, 0.7, 2.5]
    prod = ensemblestats.EnsembleProducts(thresholds, ignore_nan=True, keep=keep)
    for i, members in enumerate(leads):
        prod(DeviceArray.from_host(members) if i != 1 else members.astype(np.float64))
    assert prod.n_leadtimes == 3 and prod.received == [DeviceArray, np.ndarray, DeviceArray]
    mean, probs = prod.mean, prod.excprob
    if keep == "device":
        assert isinstance(mean, DeviceArray) and isinstance(probs, DeviceArray)
        mean, probs = mean.to_host(), probs.to_host()
    assert mean.shape == (3,) + X.shape[1:] and probs.shape == (3, 3) + X.shape[1:]
    for i, members in enumerate(leads):
        m, p = ensemblestats.products(members.astype(np.float64), thresholds, ignore_nan=True)
        assert same_bits(mean[i], m) and same_bits(probs[i], p)
        assert same_bits(mean[i], restated.mean(members.astype(np.float64)))
    only = ensemblestats.EnsembleProducts([], keep=keep)
    only(DeviceArray.from_host(X))
    assert only.excprob is None and only.mean.shape == (1,) + X.shape[1:]


def test_steps_end_to_end_with_the_device_callback(ref_pysteps):
    """The real pysteps.nowcasts.steps with the resident loop: ONE run whose callback products equal the reference's
    mean / excprob of the block the same run returned; a second run with return_output=False downloads no member; a
    plain function callback still gets the host stack."""
    from pysteps import nowcasts
    from pysteps.postprocessing import ensemblestats as ref

    from pysteps_amd import register
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.nowcasts import utils as loop
    from pysteps_amd.postprocessing import ensemblestats
    from test_callers_gpu import _steps_inputs, _steps_kwargs

    frames, V = _steps_inputs(256, 256)
    kw = _steps_kwargs()
    kw["probmatching_method"] = "cdf"
    thresholds = [-5.0, 0.0, 5.0]  # dBR
    n_leadtimes, n_members = 3, kw["n_ens_members"]
    steps = nowcasts.get_method("steps")
    try:
        register.register(patch_main_loop=True)
        prod = ensemblestats.EnsembleProducts(thresholds, ignore_nan=True, mean_ignore_nan=True)
        block = steps(frames, V, n_leadtimes, extrap_method="semilagrangian_hip", callback=prod, return_output=True, **kw)
        assert block.shape == (n_members, n_leadtimes, 256, 256) and block.dtype == np.float64
        assert prod.n_leadtimes == n_leadtimes and prod.received == [DeviceArray] * n_leadtimes
        mean, probs = prod.mean, prod.excprob
        assert mean.shape == (n_leadtimes, 256, 256) and probs.shape == (n_leadtimes, 3, 256, 256)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            for t in range(n_leadtimes):
                assert same_bits(mean[t], ref.mean(block[:, t], ignore_nan=True))
                assert same_bits(probs[t], ref.excprob(block[:, t], thresholds, ignore_nan=True))
        finite = probs[np.isfinite(probs)]
        assert np.isfinite(mean).any() and 0.0 < finite.mean() < 1.0

        quiet = ensemblestats.EnsembleProducts(thresholds, ignore_nan=True, mean_ignore_nan=True)
        out = steps(frames, V, n_leadtimes, extrap_method="semilagrangian_hip", callback=quiet, return_output=False, **kw)
        assert out is None
        assert "download" not in loop.last_run_stats and "advect" in loop.last_run_stats
        assert quiet.n_leadtimes == n_leadtimes and quiet.received == [DeviceArray] * n_leadtimes
        assert quiet.mean.shape == mean.shape and np.isfinite(quiet.mean).any()

        seen = []

        def plain(members):
            seen.append((type(members), members.shape, members.dtype))

        steps(frames, V, n_leadtimes, extrap_method="semilagrangian_hip", callback=plain, return_output=True, **kw)
        assert seen == [(np.ndarray, (n_members, 256, 256), np.dtype(np.float64))] * n_leadtimes
        assert "download" in loop.last_run_stats
    finally:
        register.unpatch_main_loop()


def test_device_callback_gets_the_host_stack_outside_the_resident_loop(ref_pysteps):
    """accepts_device changes nothing where the loop does not run the resident update: the callback gets ndarrays."""
    from pysteps import nowcasts

    from pysteps_amd import register
    from pysteps_amd.nowcasts import utils as loop
    from pysteps_amd.postprocessing import ensemblestats
    from test_callers_gpu import _steps_inputs, _steps_kwargs

    frames, V = _steps_inputs(128, 128)
    kw = _steps_kwargs()
    prod = ensemblestats.EnsembleProducts([0.0])
    try:
        register.register(patch_main_loop=True)
        loop.resident_update_enabled = False
        block = nowcasts.get_method("steps")(frames, V, 2, extrap_method="semilagrangian_hip", callback=prod, **kw)
    finally:
        loop.resident_update_enabled = True
        register.unpatch_main_loop()
    assert prod.received == [np.ndarray] * 2
    for t in range(2):
        assert same_bits(prod.mean[t], restated.mean(block[:, t]))
        assert same_bits(prod.excprob[t], restated.excprob(block[:, t], [0.0]))
