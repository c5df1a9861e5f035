"""The fractions skill score on the device (``pysteps_amd.verification.spatialscores``, csrc/fss.hip).

The kernels return the three sums behind the score as integers, so they are held to the integer restatement of
tests/helpers/fss.py with no tolerance: equal as integers.  The scores are held to the unmodified reference's - the
goldens of tests/golden/fss_reference.npz and the real package from oracle/_ref - within 5 x the deviation of the
reference's float filter from the exact integers that tools/make_golden_fss.py measured (see tests/test_fss_cpu.py).
"""

import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import fss as restated

pytestmark = pytest.mark.gpu

PATH = os.path.join(GOLDEN, "fss_reference.npz")
GPU_SCALES = [1, 2, 3, 16, 64, 255]


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def case_names():
    return [str(c) for c in np.load(PATH)["cases"]]


def bar_fss(golden):
    return 5.0 * float(golden["deviation_fss"])


def as_ints(counts):
    return [int(c) for c in np.asarray(counts).reshape(-1)]


def exact_ints(f, o, thrs, scales):
    return [int(c) for c in restated.sums_table(f, o, thrs, scales).reshape(-1)]


@pytest.mark.parametrize("resident", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", case_names())
def test_goldens_sums_equal_as_integers_and_scores_within_the_bar(golden, name, dtype, resident):
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import spatialscores

    f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
    thrs, scales = [float(t) for t in golden["thresholds"]], [int(s) for s in golden["scales"]]
    args = (DeviceArray.from_host(f), DeviceArray.from_host(o)) if resident else (f, o)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        scores, counts = spatialscores.fss_table(args[0], args[1], thrs, scales, return_sums=True)
    assert counts.shape == (3, 9, 3) and counts.dtype == np.uint64 and isinstance(scores, np.ndarray)
    assert as_ints(counts) == exact_ints(f, o, thrs, scales)
    want = golden["%s__%s__fss" % (name, dtype)]
    assert np.array_equal(np.isnan(scores), np.isnan(want))
    ok = ~np.isnan(want)
    worst = float(np.max(np.abs(scores[ok] - want[ok]), initial=0.0))
    print("%s %s: FSS within %.3g of the golden (bar %.3g)" % (name, dtype, worst, bar_fss(golden)))
    assert worst <= bar_fss(golden)
    if name.startswith("same"):
        assert np.all(scores == 1.0)
    if name.startswith("dry"):
        assert np.isnan(scores).all()
        with pytest.warns(RuntimeWarning):
            assert np.isnan(spatialscores.fss(args[0], args[1], 0.5, 8))
    else:
        one = spatialscores.fss(args[0], args[1], thrs[1], scales[4])
        assert isinstance(one, np.float64) and one == scores[1, 4]
    if not resident:
        assert np.array_equal(f, golden[name + "__f"].astype(dtype), equal_nan=True)  # the input is not modified


@pytest.mark.parametrize("shape,dtype,K", [((4096, 4096), "float32", 2), ((1226, 761), "float64", 3), ((1226, 761), "float32", 3),
                                           ((640, 710), "float32", 6), ((640, 710), "float64", 2)])
def test_generated_fields_equal_as_integers(shape, dtype, K):
    """Stacks of generated fields against a shared observation and against a stack of observations; several scales and
    thresholds in one call equal one call each."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import spatialscores

    m, n = shape
    pairs = [restated.pair(m, n, 10 * K + k, dtype) for k in range(K)]
    fct, obs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    thrs = [0.5, 0.7] if m < 4096 else [0.7]
    dev_f, dev_o = DeviceArray.from_host(fct), DeviceArray.from_host(obs)
    _, stacked = spatialscores.fss_table(dev_f, dev_o, thrs, GPU_SCALES, return_sums=True)
    want = restated.sums_table(fct, obs, thrs, GPU_SCALES)
    assert stacked.shape == (K, len(thrs), len(GPU_SCALES), 3) and as_ints(stacked) == [int(c) for c in want.reshape(-1)]
    _, shared = spatialscores.fss_table(dev_f, dev_o.view(0), thrs, GPU_SCALES, return_sums=True)
    assert as_ints(shared[0]) == as_ints(stacked[0])
    members = range(1, K) if m < 4096 else [1]
    for k in members:
        assert as_ints(shared[k]) == exact_ints(fct[k], obs[0], thrs, GPU_SCALES)
    assert len({int(c) for c in shared[:, :, :, 2].reshape(K, -1)[:, 0]}) == 1  # one observation: one sum of its squares
    # one call each
    for i, thr in enumerate(thrs):
        for j, scale in enumerate(GPU_SCALES):
            _, single = spatialscores.fss_table(dev_f.view(K - 1), dev_o.view(K - 1), thr, scale, return_sums=True)
            assert single.shape == (1, 1, 3) and as_ints(single) == as_ints(stacked[K - 1, i, j])
    # NumPy in, the same integers
    if m < 4096:
        _, host = spatialscores.fss_table(fct, obs, thrs, GPU_SCALES, return_sums=True)
        assert np.array_equal(host, stacked)
        # mixed dtypes: every field is compared in its own
        other = np.float64 if dtype == "float32" else np.float32
        _, mixed = spatialscores.fss_table(fct[0], obs[0].astype(other), thrs, [3, 64], return_sums=True)
        assert as_ints(mixed) == exact_ints(fct[0], obs[0].astype(other), thrs, [3, 64])


def test_many_scales_and_every_pass_width():
    """9 scales are a pass of 8 and a pass of 1; 7 are 4 + 2 + 1; unsorted and repeated scales keep their places."""
    from pysteps_amd.verification import spatialscores

    f, o = restated.pair(333, 517, 5)
    for scales in (restated.SCALES, [255, 1, 8, 8, 2, 128, 0], [5, 4], [255]):
        _, counts = spatialscores.fss_table(f, o, [0.5, 4.0, 0.7], scales, return_sums=True)
        assert as_ints(counts) == exact_ints(f, o, [0.5, 4.0, 0.7], scales)


def test_threshold_type_decides_as_in_numpy(golden):
    """On a float32 stack a Python float is compared as float32 and a numpy.float64 as float64: float32(0.7) >= 0.7
    holds for the first and not for the second, as in NumPy."""
    from pysteps_amd.verification import spatialscores

    f, o = golden["p640x710__f"], golden["p640x710__o"]
    assert (f == np.float32(0.7)).any()
    a_score, a = spatialscores.fss_table(f, o, 0.7, 16, return_sums=True)
    b_score, b = spatialscores.fss_table(f, o, np.float64(0.7), 16, return_sums=True)
    assert as_ints(a) == list(restated.sums(f, o, 0.7, 16)) and as_ints(b) == list(restated.sums(f, o, np.float64(0.7), 16))
    assert as_ints(a) != as_ints(b) and a_score != b_score
    assert spatialscores.fss(f, o, 0.7, 16) == a_score[0, 0] and spatialscores.fss(f, o, np.float64(0.7), 16) == b_score[0, 0]
    _, wide = spatialscores.fss_table(f.astype(np.float64), o.astype(np.float64), 0.7, 16, return_sums=True)
    assert as_ints(wide) == as_ints(b)


def test_real_reference_at_1024_directly_and_registered(golden, ref_pysteps):
    from pysteps import verification as ref_verification

    from pysteps_amd import register, verification
    from pysteps_amd.verification import spatialscores

    bar = bar_fss(golden)
    f, o = restated.pair(1024, 1024, 77, np.float64)
    f32, o32 = f.astype(np.float32), o.astype(np.float32)
    settings = [(0.5, 1), (0.7, 2), (0.7, 16), (4.0, 64), (0.5, 255)]
    ref_fss = ref_verification.get_method("fss")
    assert ref_fss is not spatialscores.fss
    want = [ref_fss(f, o, thr, scale) for thr, scale in settings]
    want32 = [ref_fss(f32, o32, thr, scale) for thr, scale in settings[:3]]
    assert 0.0 < min(want) and max(want) < 1.0 and len(set(want)) == len(want)
    got = [verification.get_method("fss")(f, o, thr, scale) for thr, scale in settings]
    got32 = [spatialscores.fss(f32, o32, thr, scale) for thr, scale in settings[:3]]
    worst = max(abs(g - w) for g, w in zip(got + got32, want + want32))
    print("1024 x 1024: FSS within %.3g of the real reference (bar %.3g)" % (worst, bar))
    assert worst <= bar
    try:
        assert "verification:fss" in register.register(fss=True)
        patched = ref_verification.get_method("fss")
        assert patched is spatialscores.fss
        assert [patched(f, o, thr, scale) for thr, scale in settings] == got
        # the reference's own accumulate-and-merge calls now count on the device
        from pysteps.verification import spatialscores as ref

        a, b = ref.fss_init(0.5, 16), ref.fss_init(0.5, 16)
        ref.fss_accum(a, f, o)
        ref.fss_accum(b, o, f)
        both = ref.fss_compute(ref.fss_merge(a, b))
        assert abs(both - ref_fss(f, o, 0.5, 16)) <= bar
        with pytest.warns(UserWarning, match="running the reference's function"):
            far = patched(f[:300, :300], o[:300, :300], 0.5, 300)
        assert far == ref_fss(f[:300, :300], o[:300, :300], 0.5, 300)
    finally:
        register.unpatch_fss()
        register.unregister_fft()
    assert ref_verification.get_method("fss") is ref_fss


def test_entry_point_refuses_what_it_does_not_count():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import spatialscores

    f = DeviceArray.from_host(np.zeros((8, 9), np.float32))
    for scales in ([256], [2.5]):
        with pytest.raises(NotImplementedError):
            spatialscores._sums(f, f, 1, 8, 9, True, [0.5], [0.5], scales)
    with pytest.raises(NotImplementedError):
        spatialscores.fss(f, f, 0.5, 300)  # resident fields cannot go to the reference
    assert as_ints(spatialscores._sums(f, f, 1, 8, 9, True, [-1.0], [-1.0], [0.5, 1, 3])) == [72, 72, 72] * 2 + [
        int((restated.window_counts(np.ones((8, 9), bool), 3) ** 2).sum())] * 3


def test_accumulator_inside_a_real_steps_run(ref_pysteps):
    """The real pysteps.nowcasts.steps with the resident loop: the accumulator receives the members where they lie, and
    its objects equal fss_accum over the members the same run returned; with return_output=False no member is
    downloaded."""
    from pysteps import nowcasts

    from pysteps_amd import register
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.nowcasts import utils as loop
    from pysteps_amd.verification import spatialscores
    from test_callers_gpu import _steps_inputs, _steps_kwargs

    frames, V = _steps_inputs(256, 256)
    kw = _steps_kwargs()
    n_leadtimes, n_members = 3, kw["n_ens_members"]
    observations = np.stack([np.roll(frames[-1], (2 * (t + 1), 3 * (t + 1)), axis=(0, 1)) for t in range(n_leadtimes)])
    thrs, scales = [-5.0, 0.0, 5.0], [1, 4, 16, 64]  # dBR
    steps = nowcasts.get_method("steps")
    try:
        register.register(patch_main_loop=True)
        acc = spatialscores.FssAccumulator(observations, thrs, scales, per_member=True)
        block = steps(frames, V, n_leadtimes, extrap_method="semilagrangian_hip", callback=acc, return_output=True, **kw)
        assert block.shape == (n_members, n_leadtimes, 256, 256) and block.dtype == np.float64
        assert acc.n_leadtimes == n_leadtimes and acc.received == [DeviceArray] * n_leadtimes
        scores = acc.fss
        assert scores.shape == (n_leadtimes, 3, 4) and acc.member_fss.shape == (n_leadtimes, n_members, 3, 4)
        for t in range(n_leadtimes):
            for i, thr in enumerate(thrs):
                for j, scale in enumerate(scales):
                    want = spatialscores.fss_init(thr, scale)
                    for k in range(n_members):
                        spatialscores.fss_accum(want, block[k, t], observations[t])
                        counts = restated.sums(block[k, t], observations[t], thr, scale)
                        assert acc.member_fss[t, k, i, j] == restated.score(counts, scale)
                    assert acc.objects[t][i][j] == want and scores[t, i, j] == spatialscores.fss_compute(want)
        assert np.isfinite(scores).all() and 0.0 < scores.min() and scores.max() < 1.0  # the case is not trivial

        quiet = spatialscores.FssAccumulator(DeviceArray.from_host(observations), thrs, scales)
        out = steps(frames, V, n_leadtimes, extrap_method="semilagrangian_hip", callback=quiet, return_output=False, **kw)
        assert out is None
        assert "download" not in loop.last_run_stats and "callback" in loop.last_run_stats
        assert quiet.received == [DeviceArray] * n_leadtimes and quiet.member_fss is None
        assert quiet.fss.shape == scores.shape and np.isfinite(quiet.fss).all()
    finally:
        register.unpatch_main_loop()
        register.unregister_fft()
