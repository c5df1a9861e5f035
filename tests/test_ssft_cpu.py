"""The short-space Fourier (ssft / nested) noise without a device: the NumPy restatement of the half-spectrum route
against the goldens of the unmodified reference, the host geometry (rectangles, mask tiles, wet-area integers, maps)
against the reference's own, the argument checks, the registration and the rules by which a call goes to the reference."""

import json
import os
import warnings

import numpy as np
import pytest

from helpers import ssft as hs

ALL_CASES = dict(hs.SSFT_CASES, **hs.NESTED_CASES)


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


def test_goldens_hold_the_documented_keys(golden, bars):
    assert sorted(golden["cases"]) == sorted(ALL_CASES)
    for name, (shape, nr, kind, kw) in ALL_CASES.items():
        field, stored_kw, planes, plane_of = _case(golden, name)
        assert np.array_equal(field, hs.field(shape, nr, kind)) and stored_kw == kw
        assert max(shape) <= 96 and planes.dtype == np.float64 and planes.shape[1:] == shape
        assert plane_of.max() == len(planes) - 1 and np.all(np.isfinite(planes))
        assert str(golden[hs.key(name, "kind")]) == ("ssft" if name in hs.SSFT_CASES else "nested")
    for name in hs.NOISE_CASES:
        for seed in hs.NOISE_SEEDS:
            noise = golden[hs.key(name, "noise_%d" % seed)]
            assert noise.shape == ALL_CASES[name][0] and abs(noise.mean()) < 1e-12 and abs(noise.std() - 1) < 1e-12
    assert 0.0 < bars["deviation_filter"] < 1e-13 and 0.0 < bars["deviation_noise"] < 1e-12
    assert os.path.getsize(hs.GOLDEN_FILE) < (1 << 20)


def test_the_cases_cover_what_they_are_there_for(golden):
    """One window just above and one just below war_thr, an all-dry bank of one plane, a nested bank with a merge at
    both levels, a partial last window."""
    field, kw, planes, plane_of = _case(golden, "war_edge")
    counts, rects = golden[hs.key("war_edge", "counts")], golden[hs.key("war_edge", "rects")]
    area = (rects[:, 1] - rects[:, 0]) * (rects[:, 3] - rects[:, 2])
    assert counts[0] - kw["war_thr"] * area[0] == 3 and counts[1] - kw["war_thr"] * area[1] == -3
    assert plane_of[0, 0] != plane_of[0, 1] and plane_of[0, 1] == plane_of[1, 0] == plane_of[1, 1]
    assert len(_case(golden, "all_dry")[2]) == 1
    assert len(_case(golden, "n64x64")[2]) == 4 and len(_case(golden, "n_level0")[2]) == 1
    rects = golden[hs.key("s80x72", "rects")]
    assert rects[-1].tolist() == [54, 80, 54, 72]  # int(64 - 9.6) .. the domain's edge: 26 x 18 of 51 x 51


@pytest.mark.parametrize("name", sorted(hs.SSFT_CASES))
def test_restated_ssft_filters_reproduce_the_reference(golden, bars, name):
    from pysteps_amd.noise import ssft as geo

    field, kw, planes, plane_of = _case(golden, name)
    half, got_map, counts, rects = hs.ssft_bank(field, **kw)
    # integers, rectangles and the map: exactly the reference's
    assert np.array_equal(rects, golden[hs.key(name, "rects")])
    assert np.array_equal(counts.ravel(), golden[hs.key(name, "counts")])
    for a in range(got_map.size):  # windows that share a plane here hold the same plane there
        for b in range(got_map.size):
            if got_map.flat[a] == got_map.flat[b]:
                assert plane_of.flat[a] == plane_of.flat[b]
    nr = 1 if field.ndim == 2 else field.shape[0]
    dry = [not float(c) / (int(r[1] - r[0]) * int(r[3] - r[2]) * nr) > kw.get("war_thr", 0.1) for c, r in zip(counts.ravel(), rects)]
    assert np.array_equal(got_map == 0, np.asarray(dry).reshape(got_map.shape))
    full = geo.expand_half(half, field.shape[-1])[got_map]
    dev = hs.plane_deviation(full, planes[plane_of])
    bar = hs.filter_bar(bars, field.shape[-2:], float(golden[hs.key(name, "amp")]))
    print("%s: filter deviation %.3g, bar %.3g" % (name, dev, bar))
    assert dev <= bar


@pytest.mark.parametrize("name", sorted(hs.NESTED_CASES))
def test_restated_nested_filters_reproduce_the_reference(golden, bars, name):
    from pysteps_amd.noise import ssft as geo

    field, kw, planes, plane_of = _case(golden, name)
    half, counts = hs.nested_bank(field, **kw)
    levels = geo.nested_levels(field.shape, kw["max_level"])
    rects = np.array([e[0] for entries in levels for e in entries], dtype=np.int64).reshape(-1, 4)
    assert np.array_equal(rects, golden[hs.key(name, "rects")])
    assert np.array_equal(np.concatenate(counts) if counts else np.zeros(0, np.int64), golden[hs.key(name, "counts")])
    dev = hs.plane_deviation(geo.expand_half(half, field.shape[-1]), planes[plane_of])
    bar = hs.filter_bar(bars, field.shape[-2:], float(golden[hs.key(name, "amp")]))
    print("%s: filter deviation %.3g, bar %.3g" % (name, dev, bar))
    assert dev <= bar


@pytest.mark.parametrize("name", hs.NOISE_CASES)
def test_restated_generator_reproduces_the_reference(golden, bars, name):
    from pysteps_amd.noise import ssft as geo

    field, kw, planes, plane_of = _case(golden, name)
    for seed in hs.NOISE_SEEDS:
        white = np.random.RandomState(seed).randn(*field.shape)
        got = hs.generate(geo.fold_half(planes), plane_of, white)
        dev = hs.field_deviation(got, golden[hs.key(name, "noise_%d" % seed)])
        bar = hs.noise_bar(bars, field.shape, float(golden[hs.key(name, "gain_%d" % seed)]))
        print("%s seed %d: noise deviation %.3g, bar %.3g" % (name, seed, dev, bar))
        assert dev <= bar


def test_fold_and_expand_are_inverse_on_symmetric_planes():
    from pysteps_amd.noise import ssft as geo

    rng = np.random.RandomState(0)
    for m, n in ((6, 8), (5, 7), (8, 5), (7, 6)):
        F = rng.rand(2, 3, m, n)
        half = geo.fold_half(F)
        mirrored = F[..., (-np.arange(m)) % m, :][..., (-np.arange(n)) % n]
        assert half.shape == (2, 3, m, n // 2 + 1) and np.array_equal(half, ((F + mirrored) / 2)[..., : n // 2 + 1])
        full = geo.expand_half(half, n)
        assert np.array_equal(full, (F + mirrored) / 2)  # the symmetric part, every bin
        assert np.array_equal(geo.fold_half(full), half)


def test_window_functions_and_masks_are_the_references(ref_pysteps):
    from pysteps.noise import fftgenerators as ref
    from pysteps.utils.tapering import compute_window_function

    from pysteps_amd.noise import ssft as geo

    for m, n in ((20, 15), (26, 18), (51, 51), (17, 22), (64, 48)):
        for func in ("tukey", "hann"):
            assert np.array_equal(geo.window_function(m, n, func), compute_window_function(m, n, func))
            mask = ref._get_mask((m + 3, n + 2), (1, m + 1), (2, n + 2), func)
            assert np.array_equal(mask[1:m + 1, 2:n + 2], geo.mask_tile(m, n, func))
    assert geo.mask_tile(4, 4, None) is None
    with pytest.raises(ValueError, match="invalid window function 'box'"):
        geo.window_function(4, 4, "box")
    # _split_field and the merge weights (DC bin: 1 / 0 = inf, weight 1)
    for seg in (2, 4):
        a, b = geo.split_field((0, 70), (0, 90), seg)
        ra, rb = ref._split_field((0, 70), (0, 90), seg)
        assert np.array_equal(a, ra) and np.array_equal(b, rb)
    w = geo.merge_weights((70, 90), 1.0, 35)
    fx, fy = np.meshgrid(np.fft.fftfreq(90, 1.0), np.fft.fftfreq(70, 1.0))
    with np.errstate(divide="ignore"):
        want = 1 / (1 + np.exp(-0.05 * (1 / np.sqrt(fx ** 2 + fy ** 2) - 35 / 2.0 * 1.0)))
    assert w[0, 0] == 1.0 and np.array_equal(w, want[:, :46])


def _bad_filter(shape=(2, 2, 8, 8), fill=1.0):
    return {"field": np.full(shape, fill), "input_shape": shape[-2:], "use_full_fft": True}


def test_argument_checks_and_messages_are_the_references(ref_pysteps):
    """None of these reaches a device."""
    from pysteps.noise import fftgenerators as ref

    from pysteps_amd.noise import fftgenerators as ours

    def message(fn, *args, **kwargs):
        with pytest.raises((ValueError, NotImplementedError)) as exc:
            fn(*args, **kwargs)
        return type(exc.value), str(exc.value)

    nan_field = np.ones((8, 8))
    nan_field[2, 3] = np.nan
    for name in ("initialize_nonparam_2d_ssft_filter", "initialize_nonparam_2d_nested_filter"):
        for bad in (np.ones(8), np.ones((2, 2, 8, 8)), nan_field):
            assert message(getattr(ours, name), bad) == message(getattr(ref, name), bad)
    gen = "generate_noise_2d_ssft_filter"
    for F, kw in ((_bad_filter((8, 8)), {}), (_bad_filter(fill=np.inf), {}), (_bad_filter(fill=np.nan), {}),
                  (_bad_filter(), {"domain": "spectral"})):
        state = np.random.get_state()
        assert message(getattr(ours, gen), F, **kw) == message(getattr(ref, gen), F, **kw)
        after = np.random.get_state()
        assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert message(getattr(ours, gen), _bad_filter(), domain="spectral")[0] is NotImplementedError


def test_registration_adds_the_two_names_and_leaves_the_stock_ones(ref_pysteps):
    import pysteps.noise.interface as noise_if
    from pysteps.noise import fftgenerators as ref

    from pysteps_amd import register
    from pysteps_amd.noise import ssft

    stock = {name: noise_if._noise_methods[name] for name in ("ssft", "nested", "nonparametric")}
    register.register()
    assert noise_if._noise_methods["ssft_hip"] == (ssft.initialize_nonparam_2d_ssft_filter, ssft.generate_noise_2d_ssft_filter)
    assert noise_if._noise_methods["nested_hip"] == (ssft.initialize_nonparam_2d_nested_filter, ssft.generate_noise_2d_ssft_filter)
    from pysteps import noise

    assert noise.get_method("ssft_hip")[0] is ssft.initialize_nonparam_2d_ssft_filter
    for name, pair in stock.items():
        assert noise_if._noise_methods[name] == pair
    assert noise_if._noise_methods["ssft"] == (ref.initialize_nonparam_2d_ssft_filter, ref.generate_noise_2d_ssft_filter)
    assert noise_if._noise_methods["nested"] == (ref.initialize_nonparam_2d_nested_filter, ref.generate_noise_2d_ssft_filter)
    assert "ssft_hip" not in register.NOISE_NAMES and "nested_hip" not in register.NOISE_NAMES
    assert set(register.SSFT_NAMES) == {"ssft_hip", "nested_hip"}


def _spied(monkeypatch):
    """the reference function replaced by a recorder: what the declining rules hand over, no device, no work"""
    from pysteps_amd.noise import ssft as hip_mod

    calls = []

    def looked_up(module, name, ours):
        def spy(*args, **kwargs):
            calls.append((module, name, args, kwargs))
            return "from the reference"

        return spy

    monkeypatch.setattr(hip_mod, "lookup", looked_up)
    return hip_mod, calls


@pytest.mark.parametrize("why", ["float32", "shape", "budget"])
@pytest.mark.parametrize("which", ["ssft", "nested"])
def test_declined_initialiser_calls_go_to_the_reference_with_a_warning(monkeypatch, which, why):
    hip_mod, calls = _spied(monkeypatch)
    field = np.ones((16, 16))
    if why == "float32":
        field, match = field.astype(np.float32), "float32"
    elif why == "shape":
        field, match = np.ones((4100, 4)), "do not take the shape"
    else:
        monkeypatch.setattr(hip_mod, "BANK_BYTES", 0)
        match = "memory budget"
    name = "initialize_nonparam_2d_%s_filter" % which
    with pytest.warns(RuntimeWarning, match=match):
        out = getattr(hip_mod, name)(field, win_fun="hann", war_thr=0.2, resident=True)
    assert out == "from the reference" and len(calls) == 1
    module, looked, args, kwargs = calls[0]
    assert (module, looked) == ("noise.fftgenerators", name) and args[0] is field
    assert kwargs == {"win_fun": "hann", "war_thr": 0.2}  # `resident` is ours alone


@pytest.mark.parametrize("why", ["float32", "shape", "budget"])
def test_declined_generator_calls_go_to_the_reference_with_a_warning(monkeypatch, why):
    hip_mod, calls = _spied(monkeypatch)
    F = _bad_filter((2, 2, 16, 16))
    if why == "float32":
        F["field"], match = F["field"].astype(np.float32), "float32"
    elif why == "shape":
        F, match = _bad_filter((1, 1, 4100, 4)), "do not take the shape"
    else:
        monkeypatch.setattr(hip_mod, "BANK_BYTES", 0)
        match = "memory budget"
    rs = np.random.RandomState(3)
    with pytest.warns(RuntimeWarning, match=match):
        out = hip_mod.generate_noise_2d_ssft_filter(F, rs, overlap=0.1)
    assert out == "from the reference" and len(calls) == 1
    module, looked, args, kwargs = calls[0]
    assert (module, looked) == ("noise.fftgenerators", "generate_noise_2d_ssft_filter") and args == (F,)
    assert kwargs == {"randstate": rs, "seed": None, "overlap": 0.1}
    before = np.random.RandomState(3).get_state()
    assert np.array_equal(rs.get_state()[1], before[1])  # nothing drawn: the reference draws for itself


def test_without_pysteps_a_declined_call_raises(monkeypatch):
    from pysteps_amd.noise import ssft as hip_mod

    monkeypatch.setattr(hip_mod, "lookup", lambda module, name, ours: None)
    with pytest.raises(NotImplementedError, match="float32"):
        hip_mod.initialize_nonparam_2d_ssft_filter(np.ones((16, 16), np.float32))
    with pytest.raises(NotImplementedError, match="do not take the shape"):
        hip_mod.generate_noise_2d_ssft_filter(_bad_filter((1, 1, 4100, 4)))


def test_the_other_callers_keep_declining_these_generators():
    """compute_noise_stddev_adjs does not take the ssft generator, the reference's or ours (the resident member loop
    likewise: tests/test_noise_adj_cpu.py and the resident loop's tests assert the stock one)."""
    from pysteps_amd.cascade.decomposition import decomposition_fft
    from pysteps_amd.noise import ssft, utils

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        reason = utils._decline_reason(np.ones((16, 16)), 0.0, {}, decomposition_fft, {}, ssft.generate_noise_2d_ssft_filter, 3,
                                       True)
    assert "noise_generator" in reason
