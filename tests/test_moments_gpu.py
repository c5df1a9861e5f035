"""The (mean, population std) reduction of whole planes on the device (``psh::moments``, csrc/noise_adj.hip) against
the wide oracle of tests/helpers/moments.py, on the planes a one-pass sum with a shift taken from the data gets wrong:
an intense value on the plane's first pixel, an offset field with a first-pixel outlier, the highest band of a cell at
(0, 0), planes around the launch's edges, constant planes, planes with a NaN or an infinity - alone through
``prepare(..., stats_out=)`` and through its callers: the cascade decomposition (host and device-resident
statistics, field mean), the noise filter, the prepare stage.

Bars: 5 x what float64 np.mean / np.std deviate from the oracle on the same plane, relative to the plane's std, per
case and per statistic, floor 16 x 2^-53 (helpers/moments.py; the CPU test holds every std bar under the project's
recorded 8.1e-14).  What is element-wise is held to identical bits given the statistics the device used.  The worst
error / bar per family goes to moments_seen.json in the directory PYSTEPS_HIP_SEEN_DIR names (no record without it).
"""

import ctypes
import json
import os

import numpy as np
import pytest

from helpers import moments as hard

pytestmark = pytest.mark.gpu

SEEN = {}
SIGMA, MU, THR2 = 2.5, -3.0, -15.0


@pytest.fixture(scope="module", autouse=True)
def seen_record():
    yield
    where = os.environ.get("PYSTEPS_HIP_SEEN_DIR")
    if not where:
        return
    try:
        os.makedirs(where, exist_ok=True)
        with open(os.path.join(where, "moments_seen.json"), "w") as fh:
            json.dump(SEEN, fh, indent=1, sort_keys=True)
    except OSError:
        pass


def _or_skip(fn, *args):
    try:
        return fn(*args)
    except hard.OracleUnavailable as why:
        pytest.skip(str(why))


def _device_stats(planes, mask=None):
    """(stats (k, 2), prepared planes) of k planes of one size through psh_noise_adj_prepare_dev; no mask: all ones."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.noise import utils as hip_mod

    planes = [np.asarray(p, dtype=np.float64) for p in planes]
    size = planes[0].size
    fields = DeviceArray.from_host(np.stack([p.reshape(-1) for p in planes]))
    if mask is None:
        d_mask = DeviceArray((size,), np.uint8).fill_bytes(1)
    else:
        d_mask = DeviceArray.from_host(np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1))
    stats = DeviceArray((len(planes), 2), np.float64)
    hip_mod.prepare(fields, d_mask, SIGMA, MU, THR2, stats_out=stats)
    return stats.to_host().copy(), fields.to_host().copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _ratios(family, label, got, x, want=None):
    """error / bar of the mean and of the std of one plane, recorded under the family; printed before any assertion"""
    want = _or_skip(hard.oracle, x) if want is None else want
    (bar_mean, bar_std), _ = hard.bars(x, want)
    err_mean, err_std = hard.errors(got, want)
    ratios = (err_mean / bar_mean, err_std / bar_std)
    worst = SEEN.setdefault(family, {"mean": 0.0, "std": 0.0})
    for key, r in zip(("mean", "std"), ratios):
        worst[key] = max(worst[key], float(r)) if np.isfinite(r) and np.isfinite(worst[key]) else float("inf")
    print("  %-34s mean err %.3g bar %.3g | std err %.3g bar %.3g | got %r want %r" % (label, err_mean, bar_mean, err_std, bar_std,
                                                                                    tuple(float(v) for v in got), want))
    return ratios


def _assert_all(rows):
    bad = [(label, r) for label, r in rows if not (r[0] <= 1.0 and r[1] <= 1.0)]
    assert not bad, "error / bar of (mean, std) above 1: %s" % bad


# ---- the reduction alone ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", hard.FAMILIES)
def test_the_reduction_alone_matches_the_oracle(family):
    print()
    rows = []
    for shape in hard.SHAPES:
        x = hard.plane(family, shape)
        got = _device_stats([x])[0][0]
        label = hard.case_id(family, shape)
        rows.append((label, _ratios(family, label, got, x, _or_skip(hard.case_oracle, family, shape))))
    _assert_all(rows)


@pytest.mark.parametrize("family", ["spike_first", "benign"])
def test_plane_sizes_across_the_edges_of_the_launch(family):
    """one lane, one wave, one block, one full grid stride of 512 x 256 elements - each one short, exact and one over"""
    print()
    rows = []
    for size in hard.EDGE_SIZES:
        x = hard.plane(family, (size,))
        got = _device_stats([x])[0][0]
        label = hard.case_id(family, (size,))
        rows.append((label, _ratios(family + "_edge_sizes", label, got, x, _or_skip(hard.case_oracle, family, (size,)))))
        if size == 1:
            assert got[0] == x[0] and got[1] == 0.0, got
    _assert_all(rows)


@pytest.mark.parametrize("shape", hard.SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_prepare_stage_on_hard_planes_is_the_numpy_expression(shape):
    """utils.py:113-118 on the hard planes, under a mask: with the std the device divided by, every value has the bits
    of the NumPy expression (the assertion of test_noise_adj_gpu.py::test_prepare_stage_is_the_numpy_expression)"""
    mask = np.random.default_rng(7).random(shape) < 0.4
    mask[0, 0] = True
    families = list(hard.HARD_FAMILIES) + ["spike_middle", "benign"]
    planes = [hard.plane(f, shape) for f in families]
    used, got = _device_stats(planes, mask)
    print()
    rows = []
    for j, family in enumerate(families):
        label = "prepare " + hard.case_id(family, shape)
        rows.append((label, _ratios(family, label, used[j], planes[j], _or_skip(hard.case_oracle, family, shape))))
        N = planes[j] / used[j, 1] * SIGMA + MU
        N[~mask] = THR2
        N -= MU
        assert np.array_equal(got[j].reshape(shape), N), (family, shape, int(np.count_nonzero(got[j].reshape(shape) != N)))
    _assert_all(rows)


@pytest.mark.parametrize("shape", hard.SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_planes_pair_does_not_depend_on_the_batch(shape):
    """a benign, a hard and a non-finite plane in one call: each pair has the bits it has when sent alone, in any
    position of the batch"""
    planes = [hard.plane("benign", shape), hard.plane("spike_first", shape), hard.nonfinite_plane("nan_first", shape),
              hard.plane("corner_cell_band", shape)]
    alone = [_device_stats([p])[0][0] for p in planes]
    together = _device_stats(planes)[0]
    backwards = _device_stats(planes[::-1])[0][::-1]
    for j in range(len(planes)):
        assert np.array_equal(_bits(together[j]), _bits(alone[j])), (j, together[j], alone[j])
        assert np.array_equal(_bits(backwards[j]), _bits(alone[j])), (j, backwards[j], alone[j])
    again = _device_stats(planes)[0]
    assert np.array_equal(_bits(again), _bits(together)), "two calls differ"


@pytest.mark.parametrize("shape", hard.SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_result_does_not_depend_on_where_the_spike_lies(shape):
    """the six rolls of one plane have one mean and one std: each is within its bar of the oracle, and the six agree
    among themselves to within the (smallest) bar"""
    print()
    rows, pairs, bars = [], [], []
    want = _or_skip(hard.case_oracle, "spike_first", shape)
    for family in hard.SPIKE_ROLLS:
        x = hard.plane(family, shape)
        assert _or_skip(hard.case_oracle, family, shape)[1] == pytest.approx(want[1], rel=1e-15)
        got = _device_stats([x])[0][0]
        label = "position " + hard.case_id(family, shape)
        rows.append((label, _ratios("position_independence", label, got, x, _or_skip(hard.case_oracle, family, shape))))
        pairs.append(got)
        bars.append(hard.bars(x, want)[0])
    pairs, bars = np.array(pairs), np.array(bars)
    spread = (pairs.max(axis=0) - pairs.min(axis=0)) / want[1]
    ratios = tuple(spread / bars.min(axis=0))
    print("  spread of the six (mean, std) / std: %s, bars %s" % (spread, bars.min(axis=0)))
    worst = SEEN.setdefault("position_spread", {"mean": 0.0, "std": 0.0})
    worst["mean"], worst["std"] = max(worst["mean"], float(ratios[0])), max(worst["std"], float(ratios[1]))
    rows.append(("spread of the six positions %s" % (shape,), ratios))
    _assert_all(rows)


@pytest.mark.parametrize("shape", hard.SHAPES, ids=lambda s: "%dx%d" % s)
def test_nonfinite_planes_report_nan_like_numpy(shape):
    """a NaN in the plane: NaN mean and NaN std; an infinity: a non-finite mean and a NaN std, as np.std gives - not a
    std of 0.0; the plane's neighbours in the batch keep their bits"""
    benign, spike = hard.plane("benign", shape), hard.plane("spike_first", shape)
    clean = _device_stats([benign, spike])[0]
    print()
    bad = []
    for kind in hard.NONFINITE:
        x = hard.nonfinite_plane(kind, shape)
        with np.errstate(invalid="ignore"):
            assert np.isnan(np.std(x))
        got = _device_stats([benign, x, spike])[0]
        print("  %-14s %s: %r" % (kind, shape, tuple(float(v) for v in got[1])))
        SEEN.setdefault("nonfinite_std_is_nan", {})["%s_%dx%d" % ((kind,) + shape)] = bool(np.isnan(got[1, 1]))
        mean_ok = np.isnan(got[1, 0]) if kind.startswith("nan") else not np.isfinite(got[1, 0])
        if not (mean_ok and np.isnan(got[1, 1])):
            bad.append((kind, tuple(float(v) for v in got[1])))
        assert np.array_equal(_bits(got[[0, 2]]), _bits(clean)), (kind, got, clean)
    assert not bad, "(mean, std) of a non-finite plane, NaN std expected: %s" % bad


def test_constant_planes():
    """the mean within 2 ulp of c; the std finite, not negative and at most 4 x 2^-53 |c| (NumPy's own pairwise mean
    can leave a std of that order, tests/test_moments_cpu.py - no exact zero is demanded)"""
    print()
    bad = []
    shapes = list(hard.SHAPES) + [(n,) for n in (1, 2, 65, 257, hard.GRID_STRIDE + 1)]
    for c in hard.CONSTANTS:
        for shape in shapes:
            mean, std = _device_stats([hard.constant_plane(c, shape)])[0][0]
            off = abs(mean - c) / np.spacing(abs(c)) if c else abs(mean)
            rel = std / (hard.U * abs(c)) if c else std
            print("  c = %-22r %-12s mean off by %.2g ulp, std %.3g = %.3g x 2^-53 |c|" % (c, shape, off, std, rel))
            worst = SEEN.setdefault("constant", {"mean_ulps_of_2": 0.0, "std_of_4u": 0.0})
            worst["mean_ulps_of_2"] = max(worst["mean_ulps_of_2"], float(off) / 2.0)
            worst["std_of_4u"] = max(worst["std_of_4u"], float(rel) / 4.0) if np.isfinite(rel) else float("inf")
            if not (off <= 2.0 and np.isfinite(std) and 0.0 <= std and rel <= 4.0):
                bad.append((c, shape, mean, std))
    assert not bad, bad


# ---- through the callers ------------------------------------------------------------------------------------------------

DECOMP_CASES = [((64, 64), 4), ((128, 96), 5), ((67, 129), 4)]


def _level_rows(family, label, levels, means, stds):
    rows = []
    for k in range(levels.shape[0]):
        rows.append(("%s level %d" % (label, k), _ratios(family, "%s level %d (d = %.1f)" % (label, k, hard.first_pixel_distance(levels[k])),
                                                         (means[k], stds[k]), levels[k])))
    return rows


@pytest.mark.parametrize("centred", [False, True], ids=["cell_at_the_first_pixel", "cell_at_the_centre"])
@pytest.mark.parametrize("shape,nlevels", DECOMP_CASES, ids=["%dx%d" % c[0] for c in DECOMP_CASES])
def test_the_level_statistics_of_the_decomposition(shape, nlevels, centred):
    """decomposition_fft on -15 dB with one intense cell on pixel (0, 0) / rolled to the centre: the returned means and
    stds are the oracle's moments of the device's own returned levels (the transforms are held per bin by
    tests/test_fft_pointwise_gpu.py and are not part of this comparison); normalised levels are (raw - mean) / std with
    the returned statistics, bit for bit; the field mean of subtract_mean likewise"""
    from pysteps_amd.cascade import decomposition_fft
    from pysteps_amd.cascade.bandpass_filters import filter_gaussian

    field = hard.cell_field(shape, centred)
    bp = filter_gaussian(shape, nlevels)
    family = "decomposition_centred" if centred else "decomposition_first_pixel"
    print()
    raw = decomposition_fft(field, bp, normalize=False, compute_stats=True)
    levels = np.array(raw["cascade_levels"])
    rows = _level_rows(family, "raw %s" % (shape,), levels, raw["means"], raw["stds"])
    if not centred:
        assert max(hard.first_pixel_distance(levels[k]) for k in range(nlevels)) >= 20.0  # the case is a hard one

    normed = decomposition_fft(field, bp, normalize=True, compute_stats=True)
    assert np.array_equal(_bits(normed["means"]), _bits(raw["means"])) and np.array_equal(_bits(normed["stds"]), _bits(raw["stds"]))
    for k in range(nlevels):
        want = (levels[k] - raw["means"][k]) / raw["stds"][k]
        assert np.array_equal(normed["cascade_levels"][k], want), (k, int(np.count_nonzero(normed["cascade_levels"][k] != want)))

    centred_run = decomposition_fft(field, bp, normalize=False, compute_stats=True, subtract_mean=True)
    rows.append(("field mean", _ratios(family, "field mean %s" % (shape,), (centred_run["field_mean"], hard.oracle(field)[1]), field)))
    rows += _level_rows(family, "subtract_mean %s" % (shape,), np.array(centred_run["cascade_levels"]), centred_run["means"],
                        centred_run["stds"])
    _assert_all(rows)


@pytest.mark.parametrize("shape,nlevels", DECOMP_CASES, ids=["%dx%d" % c[0] for c in DECOMP_CASES])
def test_the_device_resident_level_statistics(shape, nlevels):
    """psh_cascade_decompose_stats_dev (what the resident member loop standardises its noise cascade with): the pairs
    left in device memory against the oracle's moments of the levels left beside them"""
    from pysteps_amd import _lib
    from pysteps_amd.cascade.bandpass_filters import filter_gaussian
    from pysteps_amd.device import DeviceArray

    m, n = shape
    weights = DeviceArray.from_host(np.ascontiguousarray(filter_gaussian(shape, nlevels)["weights_2d"], dtype=np.float64))
    print()
    rows = []
    for centred in (False, True):
        field = DeviceArray.from_host(hard.cell_field(shape, centred))
        levels, stats = DeviceArray((nlevels, m, n), np.float64), DeviceArray((nlevels, 2), np.float64)
        _lib.check(_lib.lib().psh_cascade_decompose_stats_dev(field.ptr, weights.ptr, nlevels, m, n, levels.ptr, stats.ptr),
                   "psh_cascade_decompose_stats_dev")
        got, host_levels = stats.to_host().copy(), levels.to_host().copy()
        rows += _level_rows("decomposition_resident", "resident %s centred=%s" % (shape, centred), host_levels, got[:, 0], got[:, 1])
    _assert_all(rows)


@pytest.mark.parametrize("shape", hard.SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_noise_filter_standardises_a_field_whose_first_pixel_is_its_peak(shape):
    """psh_noise_filter_dev on white noise 1e-3 N(0, 1) plus a delta at (0, 0) under a smooth radial filter: the output's
    first pixel is its peak; the oracle's mean of the output is 0 and its std 1, to within the bars of that plane"""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    m, n = shape
    white = DeviceArray.from_host(hard.delta_noise(shape))
    filt = DeviceArray.from_host(hard.radial_filter(shape))
    out = DeviceArray(shape, np.float64)
    _lib.check(_lib.lib().psh_noise_filter_dev(white.ptr, filt.ptr, m, n, out.ptr), "psh_noise_filter_dev")
    got = out.to_host().copy()
    assert np.all(np.isfinite(got)) and np.argmax(got) == 0
    mean, std = _or_skip(hard.oracle, got)
    (bar_mean, bar_std), _ = hard.bars(got, (mean, std))
    d = abs(got[0, 0] - mean) / std
    ratios = (abs(mean) / bar_mean, abs(std - 1.0) / bar_std)
    print("\n  noise filter %s: d = %.1f, oracle mean %.3g (bar %.3g), std - 1 %.3g (bar %.3g)" % (shape, d, mean, bar_mean, std - 1.0, bar_std))
    worst = SEEN.setdefault("noise_filter", {"mean": 0.0, "std": 0.0})
    worst["mean"], worst["std"] = max(worst["mean"], float(ratios[0])), max(worst["std"], float(ratios[1]))
    assert d >= 30.0
    _assert_all([("noise filter %s" % (shape,), ratios)])
