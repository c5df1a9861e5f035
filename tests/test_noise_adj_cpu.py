"""The noise standard-deviation adjustment without a device: the yardsticks (restatement, goldens), the rules by which
``pysteps_amd.noise.utils.compute_noise_stddev_adjs`` hands a call to the reference, the registration and the seed
chain."""

import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import noise_adj as restated

GOLDEN_FILE = os.path.join(GOLDEN, "noise_adj_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN_FILE, allow_pickle=False)


@pytest.fixture(scope="module")
def small_case(ref_pysteps, golden):
    R = golden["p64x64__R"].astype(np.float64)
    F, noise_filter = restated.filters(ref_pysteps, R, restated.CASES["p64x64"][1])
    return R, F, noise_filter


def test_goldens_load_and_hold_the_documented_keys(golden):
    assert sorted(golden["cases"]) == sorted(restated.CASES)
    for name, (shape, levels, seed) in restated.CASES.items():
        R32 = golden[name + "__R"]
        assert R32.dtype == np.float32 and R32.shape == shape
        assert np.array_equal(R32, restated.field(shape, seed))
    for combo in restated.all_keys():
        k = restated.key(*combo)
        levels = restated.CASES[combo[0]][1]
        assert golden[k + "__ref"].shape == (levels,) and golden[k + "__ld"].shape == (levels,)
        assert golden[k + "__ref"].dtype == np.float64 and np.all(np.isfinite(golden[k + "__ref"]))
    assert 0.0 < float(golden["deviation_coeffs"]) < 1e-10
    assert 0.0 < float(golden["deviation_moments"]) < 1e-12
    assert os.path.getsize(GOLDEN_FILE) <= max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                                                if f != os.path.basename(GOLDEN_FILE))


@pytest.mark.parametrize("name", sorted(restated.CASES))
def test_restatement_at_float64_is_the_reference_bit_for_bit(ref_pysteps, golden, name):
    from pysteps.cascade.decomposition import decomposition_fft
    from pysteps.noise.fftgenerators import generate_noise_2d_fft_filter
    from pysteps.noise.utils import compute_noise_stddev_adjs

    R = golden[name + "__R"].astype(np.float64)
    F, noise_filter = restated.filters(ref_pysteps, R, restated.CASES[name][1])
    combos = [("wet", True, 3, 0), ("wet", False, 3, 42), ("sparse", True, 3, 0), ("all", False, 3, 0)]
    if name == "p64x64":
        combos = [c[1:] for c in restated.all_keys() if c[0] == name]
    for mask_kind, conditional, num_iter, seed in combos:
        thr1, thr2 = restated.thresholds(R, mask_kind)
        before = R.copy()
        ref = compute_noise_stddev_adjs(R, thr1, thr2, F, decomposition_fft, noise_filter, generate_noise_2d_fft_filter, num_iter,
                                        conditional=conditional, seed=seed)
        got = restated.restated(R, thr1, thr2, F["weights_2d"], noise_filter["field"], num_iter, conditional, seed)
        assert np.array_equal(np.asarray(ref), got), (mask_kind, conditional, num_iter, seed)
        assert np.array_equal(R, before)
        # the stored coefficients are what the reference gives here (same NumPy) up to its own rounding noise
        stored = golden[restated.key(name, mask_kind, conditional, num_iter, seed) + "__ref"]
        assert restated.rel_dev(got, stored) <= 5 * float(golden["deviation_coeffs"])


def _spied(monkeypatch):
    """the reference function replaced by a recorder: what the declining rules hand over, no device, no work"""
    from pysteps_amd.noise import utils as hip_mod

    calls = []

    def spy(R, *args, **kwargs):
        calls.append((R, args, kwargs))
        return "from the reference"

    monkeypatch.setattr(hip_mod, "lookup", lambda module, name, ours: spy)
    return hip_mod, calls


@pytest.mark.parametrize("why", ["float32", "full_fft", "empty_wet_area", "num_iter_0", "ssft_generator"])
def test_declined_calls_go_to_the_reference_with_a_warning(ref_pysteps, small_case, monkeypatch, why):
    from pysteps.cascade.decomposition import decomposition_fft
    from pysteps.noise import fftgenerators

    hip_mod, calls = _spied(monkeypatch)
    R, F, noise_filter = small_case
    thr1, thr2 = restated.thresholds(R, "wet")
    generator, num_iter, conditional, match = fftgenerators.generate_noise_2d_fft_filter, 3, True, None
    if why == "float32":
        R, match = R.astype(np.float32), "float32"
    elif why == "full_fft":
        noise_filter, match = fftgenerators.initialize_nonparam_2d_fft_filter(R, use_full_fft=True), "use_full_fft"
    elif why == "empty_wet_area":
        thr1, match = float(R.max()) + 1.0, "wet pixels"
    elif why == "num_iter_0":
        num_iter, match = 0, "num_iter"
    else:
        generator, match = fftgenerators.generate_noise_2d_ssft_filter, "noise_generator"
    with pytest.warns(RuntimeWarning, match=match):
        out = hip_mod.compute_noise_stddev_adjs(R, thr1, thr2, F, decomposition_fft, noise_filter, generator, num_iter,
                                                conditional=conditional, num_workers=2, seed=7)
    assert out == "from the reference" and len(calls) == 1
    got_R, args, kwargs = calls[0]
    assert got_R is R and args[0] == thr1 and args[1] == thr2 and args[2] is F and args[4] is noise_filter and args[6] == num_iter
    assert kwargs == {"conditional": conditional, "num_workers": 2, "seed": 7}


def test_our_own_operators_are_recognised(small_case):
    from pysteps_amd.cascade.decomposition import decomposition_fft
    from pysteps_amd.noise import compute_noise_stddev_adjs, fftgenerators, utils as hip_mod

    assert compute_noise_stddev_adjs is hip_mod.compute_noise_stddev_adjs
    R, F, noise_filter = small_case
    assert hip_mod._decline_reason(R, -10.0, F, decomposition_fft, noise_filter, fftgenerators.generate_noise_2d_fft_filter, 20,
                                   True) is None
    assert "decomp_method" in hip_mod._decline_reason(R, -10.0, F, np.mean, noise_filter,
                                                      fftgenerators.generate_noise_2d_fft_filter, 20, True)


def test_without_pysteps_a_declined_call_raises(small_case, monkeypatch):
    from pysteps_amd.noise import utils as hip_mod

    R, F, noise_filter = small_case
    monkeypatch.setattr(hip_mod, "lookup", lambda module, name, ours: None)
    with pytest.raises(NotImplementedError, match="decomp_method"):
        hip_mod.compute_noise_stddev_adjs(R, -10.0, -15.0, F, hip_mod._is_fn, noise_filter, hip_mod._is_fn, 0)


def test_patch_and_unpatch_swap_the_attribute(ref_pysteps):
    import pysteps.noise.utils as ref_mod

    from pysteps_amd import register
    from pysteps_amd.noise import utils as hip_mod

    stock = ref_mod.compute_noise_stddev_adjs
    assert stock is not hip_mod.compute_noise_stddev_adjs
    register.register()  # (the FFT method name is only reported by the call that installs it)
    before = register.register()
    assert ref_mod.compute_noise_stddev_adjs is stock, "off by default"
    try:
        assert register.patch_noise_stddev_adj() == ["noise.utils:compute_noise_stddev_adjs"]
        assert ref_mod.compute_noise_stddev_adjs is hip_mod.compute_noise_stddev_adjs
        assert hip_mod.lookup("noise.utils", "compute_noise_stddev_adjs", hip_mod.compute_noise_stddev_adjs) is stock
        assert register.patch_noise_stddev_adj() == []
    finally:
        register.unpatch_noise_stddev_adj()
    assert ref_mod.compute_noise_stddev_adjs is stock
    assert hip_mod.lookup("noise.utils", "compute_noise_stddev_adjs", hip_mod.compute_noise_stddev_adjs) is stock
    assert not hasattr(ref_mod, "_reference_compute_noise_stddev_adjs")
    try:
        added = register.register(noise_stddev_adj=True)
        assert added == before + ["noise.utils:compute_noise_stddev_adjs"]
        assert ref_mod.compute_noise_stddev_adjs is hip_mod.compute_noise_stddev_adjs
    finally:
        register.unpatch_noise_stddev_adj()
    assert register.register() == before
    assert ref_mod.compute_noise_stddev_adjs is stock


@pytest.mark.parametrize("seed", [0, 42, 123456789])
def test_seed_chain_is_the_references(seed):
    from pysteps_amd.noise import utils as hip_mod

    ours = hip_mod._seed_chain(seed, 20)
    # the reference's loop (pysteps/noise/utils.py:103-106), written out
    theirs = []
    s = seed
    for _ in range(20):
        rs = np.random.RandomState(seed=s)
        theirs.append(rs)
        s = rs.randint(0, high=1e9)
    assert len(ours) == 20
    for a, b in zip(ours, theirs):
        sa, sb = a.get_state(legacy=True), b.get_state(legacy=True)
        assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    assert all(np.array_equal(a.get_state()[1], b.get_state()[1]) for a, b in zip(ours, restated.seed_chain(seed, 20)))


def test_seed_none_leaves_the_global_generator_alone():
    from pysteps_amd.noise import utils as hip_mod

    np.random.seed(5)
    before = np.random.get_state()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        chain = hip_mod._seed_chain(None, 3)
    after = np.random.get_state()
    assert len(chain) == 3 and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
