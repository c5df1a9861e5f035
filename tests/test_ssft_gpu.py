"""The short-space Fourier (ssft / nested) noise on the device (pysteps_amd/noise/ssft.py, csrc/ssft.hip) against the
goldens of the unmodified reference (tools/make_golden_ssft.py), every element of every filter plane and every pixel of
every noise field, within 5 x the reference's own deviation from the long-double evaluation plus the transform's bar
(helpers/ssft.py ``filter_bar`` / ``noise_bar``).  Integers, maps and generator states have no tolerance.

Figures seen on the MI355X are in the README; every test prints its own before it asserts."""

import json
import warnings

import numpy as np
import pytest

from conftest import nan_mismatch, rel_l2
from helpers import ssft as hs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(hs.GOLDEN_FILE, allow_pickle=False)


@pytest.fixture(scope="module")
def bars():
    return hs.load_bars()


def _case(golden, name):
    kw = json.loads(str(golden[hs.key(name, "kwargs")]))
    if "win_size" in kw and isinstance(kw["win_size"], list):
        kw["win_size"] = tuple(kw["win_size"])
    planes, plane_of = golden[hs.key(name, "planes")], golden[hs.key(name, "plane_of")]
    return golden[hs.key(name, "field")], kw, planes, plane_of


def _filter_of(golden, name):
    field, kw, planes, plane_of = _case(golden, name)
    return {"field": np.ascontiguousarray(planes[plane_of]), "input_shape": field.shape[-2:], "use_full_fft": True}


def _refines(a, b):
    """Windows that share a plane in ``a`` share one in ``b``."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return all(b[i] == b[j] for i in range(a.size) for j in range(a.size) if a[i] == a[j])


def _same_state(a, b):
    sa, sb = a.get_state(legacy=True), b.get_state(legacy=True)
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


@pytest.mark.parametrize("name", sorted(hs.SSFT_CASES))
def test_ssft_filters_every_element(golden, bars, name):
    from pysteps_amd.noise import fftgenerators as ours

    field, kw, planes, plane_of = _case(golden, name)
    before = field.copy()
    resident = ours.initialize_nonparam_2d_ssft_filter(field, resident=True, **kw)
    bank = resident["field"]
    assert np.array_equal(field, before)
    assert resident["use_full_fft"] is True and tuple(resident["input_shape"]) == field.shape[-2:]
    assert np.array_equal(bank.war_counts.ravel(), golden[hs.key(name, "counts")])
    assert bank.shape == planes[plane_of].shape
    assert _refines(bank.plane_of, plane_of)  # windows that share a plane here hold the same plane in the reference
    want = planes[plane_of]
    got = bank.to_full()
    dev = hs.plane_deviation(got, want)
    bar = hs.filter_bar(bars, field.shape[-2:], float(golden[hs.key(name, "amp")]))
    print("%s: filter deviation %.3g, bar %.3g, %d distinct planes" % (name, dev, bar, bank.nplanes))
    assert dev <= bar
    # the reference's dictionary: a host 4-D array of the same bits, usable by either generator
    host = ours.initialize_nonparam_2d_ssft_filter(field, **kw)
    assert isinstance(host["field"], np.ndarray) and host["field"].dtype == np.float64
    assert np.array_equal(host["field"], got) and host["use_full_fft"] is True
    if name == "all_dry":
        assert bank.nplanes == 1 and not bank.plane_of.any()


@pytest.mark.parametrize("name", sorted(hs.NESTED_CASES))
def test_nested_filters_every_element(golden, bars, name):
    from pysteps_amd.noise import fftgenerators as ours

    field, kw, planes, plane_of = _case(golden, name)
    resident = ours.initialize_nonparam_2d_nested_filter(field, resident=True, **kw)
    bank = resident["field"]
    counts = np.concatenate(bank.war_counts) if bank.war_counts else np.zeros(0, np.int64)
    assert np.array_equal(counts, golden[hs.key(name, "counts")])
    assert _refines(bank.plane_of, plane_of) and _refines(plane_of, bank.plane_of) and bank.nplanes == len(planes)  # the same sharing
    want = planes[plane_of]
    got = bank.to_full()
    assert got.shape == want.shape
    dev = hs.plane_deviation(got, want)
    bar = hs.filter_bar(bars, field.shape[-2:], float(golden[hs.key(name, "amp")]))
    print("%s: filter deviation %.3g, bar %.3g, %d distinct planes" % (name, dev, bar, bank.nplanes))
    assert dev <= bar
    host = ours.initialize_nonparam_2d_nested_filter(field, 1.0, **kw)
    assert np.array_equal(host["field"], got)


@pytest.mark.parametrize("name", hs.NOISE_CASES)
def test_generator_every_pixel_and_the_generator_state(golden, bars, name):
    from pysteps_amd.noise import fftgenerators as ours

    F = _filter_of(golden, name)
    shape = tuple(F["input_shape"])
    for seed in hs.NOISE_SEEDS:
        want = golden[hs.key(name, "noise_%d" % seed)]
        rs, twin = np.random.RandomState(seed), np.random.RandomState(seed)
        got = ours.generate_noise_2d_ssft_filter(F, randstate=rs)
        twin.randn(*shape)
        assert _same_state(rs, twin)  # left where the reference leaves it
        dev = hs.field_deviation(got, want)
        bar = hs.noise_bar(bars, shape, float(golden[hs.key(name, "gain_%d" % seed)]))
        print("%s seed %d: noise deviation %.3g, bar %.3g" % (name, seed, dev, bar))
        assert got.shape == shape and got.dtype == np.float64 and dev <= bar
        # seed= on the caller's generator and on the global one: the same stream, the same bits
        rs2 = np.random.RandomState(0)
        assert np.array_equal(ours.generate_noise_2d_ssft_filter(F, randstate=rs2, seed=seed), got) and _same_state(rs2, twin)
        kept = np.random.get_state()
        try:
            assert np.array_equal(ours.generate_noise_2d_ssft_filter(F, seed=seed), got)
            now = np.random.get_state()
            assert np.array_equal(now[1], twin.get_state()[1]) and now[2:] == twin.get_state()[2:]
        finally:
            np.random.set_state(kept)


@pytest.mark.parametrize("overlap,win_fun", [(0.2, "tukey"), (-0.1, "tukey"), (0.2, None), (0.3, "hann")])
def test_generator_folds_an_arbitrary_filter(ref_pysteps, bars, overlap, win_fun):
    """A random NON-symmetric 4-D array: only its symmetric part reaches the real part of the inverse transform.  The
    reference here is the unmodified function.  The truncated window bounds leave pixels that no window covers (sM == 0,
    the last row here; more with a negative overlap): they keep 0."""
    from pysteps.noise.fftgenerators import generate_noise_2d_ssft_filter as ref_generate

    from pysteps_amd.noise import fftgenerators as ours
    from pysteps_amd.noise import ssft as geo

    shape = (48, 40)
    rng = np.random.RandomState(11)
    F = {"field": 0.5 + rng.rand(2, 3, *shape), "input_shape": shape, "use_full_fft": True}
    kw = dict(overlap=overlap, win_fun=win_fun)
    want = ref_generate(F, randstate=np.random.RandomState(5), **kw)
    rs = np.random.RandomState(5)
    got = ours.generate_noise_2d_ssft_filter(F, randstate=rs, **kw)
    det = {}
    planes, plane_of = hs.dedupe(F["field"])
    restated = hs.generate(geo.fold_half(planes), plane_of, np.random.RandomState(5).randn(*shape), details=det, **kw)
    assert np.count_nonzero(det["sM"] == 0) >= shape[1]
    dev, dev_restated = hs.field_deviation(got, want), hs.field_deviation(restated, want)
    bar = hs.noise_bar(bars, shape, det["gain"])
    print("fold %s %s: noise deviation %.3g (restatement %.3g), bar %.3g" % (overlap, win_fun, dev, dev_restated, bar))
    assert dev <= bar


def test_runs_batches_and_bank_forms_give_the_same_bits(golden, bars):
    from pysteps_amd.noise import fftgenerators as ours
    from pysteps_amd.noise.randstate import DeviceRandomStates

    name = "s80x72"
    field, kw, planes, plane_of = _case(golden, name)
    shape = field.shape
    resident = ours.initialize_nonparam_2d_ssft_filter(field, resident=True, **kw)
    again = ours.initialize_nonparam_2d_ssft_filter(field, resident=True, **kw)
    assert np.array_equal(resident["field"].half_planes(), again["field"].half_planes())  # two runs, equal bits
    host = {"field": resident["field"].to_full(), "input_shape": shape, "use_full_fft": True}
    first = ours.generate_noise_2d_ssft_filter(resident, randstate=np.random.RandomState(3))
    assert np.array_equal(first, ours.generate_noise_2d_ssft_filter(resident, randstate=np.random.RandomState(3)))
    # the uploaded host array of the same filter: folded, deduplicated, cached - and the same bits
    assert np.array_equal(first, ours.generate_noise_2d_ssft_filter(host, randstate=np.random.RandomState(3)))
    assert np.array_equal(first, ours.generate_noise_2d_ssft_filter(host, randstate=np.random.RandomState(3)))

    # K = 3 in one call against three calls of one: bit for bit, wherever a plane lies in the batch
    seeds = (3, 4, 5)
    drs = DeviceRandomStates([np.random.RandomState(s) for s in seeds], shape[0] * shape[1], n_draws=1)
    try:
        table = ours.generate_noise_table(resident, drs, 3).to_host()
    finally:
        drs.close()
    assert table.shape == (3,) + shape
    for k, s in enumerate(seeds):
        one = DeviceRandomStates([np.random.RandomState(s)], shape[0] * shape[1], n_draws=1)
        try:
            single = ours.generate_noise_table(host, one, 1).to_host()[0]
        finally:
            one.close()
        assert np.array_equal(table[k], single)
        # and the host-drawn call: the device's randn is NumPy's up to the last bits of its logarithm
        drawn = ours.generate_noise_2d_ssft_filter(resident, randstate=np.random.RandomState(s))
        dev = hs.field_deviation(table[k], drawn)
        print("table plane %d against the host-drawn call: %.3g" % (k, dev))
        assert dev <= hs.noise_bar(bars, shape, float(golden[hs.key(name, "gain_42")]))


def test_steps_with_ssft_hip_against_the_stock_generator(ref_pysteps):
    """The real nowcasts.steps with noise_method="ssft_hip" against the same call with "ssft": the bar the caller tests
    hold a stock-versus-device operator to.  Without probability matching, which would hand out the observed field's
    own values rank by rank and hide what the noise fields differ by."""
    from pysteps import nowcasts
    from tools import synth

    from pysteps_amd import register

    register.register()
    m = n = 64
    frames = synth.steps_frames(m, n, 3).astype(np.float64)  # the device path is float64
    V = synth.true_velocity(m, n).astype(np.float64)
    kw = dict(n_ens_members=2, n_cascade_levels=4, precip_thr=-10.0, kmperpixel=1.0, timestep=5.0, seed=42,
              vel_pert_method=None, mask_method="incremental", probmatching_method=None, num_workers=1,
              noise_kwargs={"win_fun": "tukey", "win_size": (32, 32)})
    steps = nowcasts.get_method("steps")
    want = steps(frames, V, 2, noise_method="ssft", **kw)
    with warnings.catch_warnings():  # a call handed to the reference would make this comparison an empty one
        warnings.filterwarnings("error", message="pysteps_amd (initialize_nonparam|generate_noise)")
        got = steps(frames, V, 2, noise_method="ssft_hip", **kw)
    assert want.shape == (2, 2, m, n) and got.shape == want.shape
    rel = rel_l2(got, want)
    print("steps ssft_hip against ssft: rel L2 %.3g, NaN mismatches %d" % (rel, nan_mismatch(got, want)))
    assert nan_mismatch(got, want) == 0
    assert rel <= 1e-4
