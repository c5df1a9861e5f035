"""Sparse-vector QC (host NumPy product code) and its oracle against the reference's goldens.

Mirrors pysteps/tests/test_utils_cleansing.py and pins oracle/sparse.py and
pysteps_amd.utils.cleansing to outputs of the unmodified reference functions
(tests/golden/sparse_reference.npz, made by tools/make_golden.py).
"""

import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import sparse as osp
from pysteps_amd.utils import cleansing


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "sparse_reference.npz"))


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_outliers_and_decluster_match_reference(gold, case):
    xy, uv = gold[case + "/xy"], gold[case + "/uv"]
    for impl in (cleansing, osp):
        out = impl.detect_outliers(uv, 3, xy, 30)
        assert np.array_equal(out, gold[case + "/outliers"])
        dxy, duv = impl.decluster(xy[~out], uv[~out], 20, 1)
        np.testing.assert_allclose(dxy, gold[case + "/dxy"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(duv, gold[case + "/duv"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", ["a", "b"])
def test_oracle_idw_matches_reference(gold, case):
    m, n = gold[case + "/shape"]
    dxy, duv = gold[case + "/dxy"], gold[case + "/duv"]
    np.testing.assert_allclose(osp.idw(dxy, duv, m, n), gold[case + "/idw"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(
        osp.idw(dxy, duv, m, n, k=5, power=2.0, dist_offset=0.1), gold[case + "/idw_k5_p2"], rtol=0, atol=1e-12
    )


# ---- mirrors of pysteps/tests/test_utils_cleansing.py ----------------------
def test_decluster_empty():
    xy, uv = cleansing.decluster(np.empty((0, 2)), np.empty((0, 2)), 20)
    assert xy.shape == (0, 2) and uv.shape == (0, 2)


def test_decluster_single_and_median():
    c, v = cleansing.decluster(np.array([[3.0, 4.0]]), np.array([[1.0, 2.0]]), 20)
    assert np.array_equal(c, [[3.0, 4.0]]) and np.array_equal(v, [[1.0, 2.0]])
    rng = np.random.default_rng(0)
    coord = rng.uniform(0, 99, (51, 2))
    vals = rng.normal(size=(51, 2))
    c, v = cleansing.decluster(coord, vals, 100)
    assert np.allclose(v, np.median(vals, axis=0)) and np.allclose(c, np.median(coord, axis=0))
    c1, v1 = cleansing.decluster(coord, vals[:, 0], 100)
    assert v1.shape == (1, 1)
    c, v = cleansing.decluster(coord, vals, 20, min_samples=3)
    assert c.shape[0] < 25


def test_decluster_errors():
    with pytest.raises(ValueError):
        cleansing.decluster(np.ones((4, 2)), np.ones((3, 2)), 20)
    with pytest.raises(ValueError):
        cleansing.decluster(np.ones(4), np.ones((4, 2)), 20)
    with pytest.raises(ValueError):
        cleansing.decluster(np.ones((4, 2)), np.full((4, 2), np.nan), 20)
    with pytest.raises(ValueError):
        cleansing.decluster(np.ones((4, 2)), np.ones((4, 2)), np.ones(3))


def test_outliers_constant_and_planted():
    assert not cleansing.detect_outliers(np.zeros(20), 1).any()
    assert not cleansing.detect_outliers(np.zeros((20, 2)), 1).any()
    assert cleansing.detect_outliers(np.zeros((1, 2)), 1).shape == (1,)
    rng = np.random.default_rng(1)
    data = rng.normal(size=200)
    data[7] = 40.0
    flags = cleansing.detect_outliers(data, 4)
    assert flags[7] and flags.sum() == 1
    data2 = rng.normal(size=(300, 2))
    data2[11] = (30.0, -30.0)
    flags = cleansing.detect_outliers(data2, 5)
    assert flags[11] and flags.sum() == 1
    coord = rng.uniform(0, 100, (300, 2))
    flags = cleansing.detect_outliers(data2, 5, coord, 30)
    assert flags[11]
    flags = cleansing.detect_outliers(data, 4, rng.uniform(0, 100, 200), 30)
    assert flags[7]


def test_outliers_errors():
    with pytest.raises(ValueError):
        cleansing.detect_outliers(np.ones((3, 2, 2)), 1)
    with pytest.raises(ValueError):
        cleansing.detect_outliers(np.array([1.0, np.nan]), 1)
    with pytest.raises(ValueError):
        cleansing.detect_outliers(np.ones(5), 1, np.ones((4, 2)), 2)


def test_live_reference_cleansing():
    """The reference's outputs for 2 .. 700 vectors with a planted outlier (tests/golden/cleansing_reference.npz)."""
    z = np.load(os.path.join(GOLDEN, "cleansing_reference.npz"), allow_pickle=False)
    for L in (2, 5, 31, 32, 700):
        c = "L%d/" % L
        xy, uv = z[c + "xy"], z[c + "uv"]
        assert np.array_equal(cleansing.detect_outliers(uv, 3, xy, 30), z[c + "outliers_local"])
        if L > 2:  # the global test (k=None), both the product's host mirror and the oracle
            want_g = z[c + "outliers_global"]
            assert np.array_equal(cleansing.detect_outliers(uv, 2.5, xy, None), want_g)
            assert np.array_equal(osp.detect_outliers(uv, 2.5, xy, None), want_g)
            assert np.array_equal(osp.detect_outliers(uv[:, 0], 2.5, None, None), z[c + "outliers_global_1d"])
        gc, gv = cleansing.decluster(xy, uv, 20, 1)
        np.testing.assert_allclose(gc, z[c + "decluster_xy"], atol=1e-12)
        np.testing.assert_allclose(gv, z[c + "decluster_uv"], atol=1e-12)
        gc, gv = cleansing.decluster(xy, uv, [20, 35], 2)
        np.testing.assert_allclose(gc, z[c + "decluster2_xy"], atol=1e-12)
        np.testing.assert_allclose(gv, z[c + "decluster2_uv"], atol=1e-12)


def test_decluster_native_orderings():
    """psh_decluster_host orders the cells with a byte-wise radix sort over their bounding box and
    falls back to a comparison sort when the box is huge; both must give the oracle's
    lexicographic cell order, medians and min_samples filtering, also for negative and
    fractional coordinates."""
    from oracle import sparse as osp

    rng = np.random.default_rng(12)
    cases = [
        (rng.uniform(-500, 4000, (1500, 2)), 20.0, 1),       # radix path, negative cells
        (rng.uniform(0, 300, (800, 2)), 7.5, 2),             # dense cells, min_samples filter
        (rng.uniform(0, 100, (64, 2)), 0.01, 1),             # > 255 cells per axis: both byte passes
        (rng.uniform(-3e9, 3e9, (200, 2)), 3.0, 1),          # box wider than 65536 cells: fallback
        (np.repeat(rng.uniform(0, 50, (5, 2)), 4, axis=0), 20.0, 1),  # duplicates: medians of equal values
    ]
    for xy, scale, min_samples in cases:
        uv = rng.normal(0, 1, xy.shape)
        gc, gv = cleansing.decluster(xy, uv, scale, min_samples)
        wc, wv = osp.decluster(xy, uv, scale, min_samples)
        assert gc.shape == wc.shape
        assert np.array_equal(gc, wc) and np.array_equal(gv, wv)


def test_parameters_beyond_the_kernel_limits_reach_the_reference(ref_pysteps):
    """interp_kwargs / fd_kwargs the kernels do not implement (IDW with 32 < k < nsamples,
    power <= 0; Shi-Tomasi block_size even or > 7; windows > 64) must behave like stock pysteps
    when pysteps is importable - delegated with a warning, not an error from the library."""
    import warnings

    from pysteps.exceptions import MissingOptionalDependency
    from pysteps.utils.interpolate import idwinterp2d as ref_idw
    from pysteps_amd.motion.lucaskanade import dense_lucaskanade
    from pysteps_amd.utils.interpolate import idwinterp2d

    rng = np.random.default_rng(5)
    xy = np.column_stack([rng.integers(0, 60, 120), rng.integers(0, 50, 120)]).astype(float)
    uv = rng.normal(0, 1, (120, 2))
    xg, yg = np.arange(60), np.arange(50)
    for kw in (dict(k=50), dict(power=0.0), dict(power=-1.0, k=10)):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = idwinterp2d(xy, uv, xg, yg, **kw)
        assert any("delegating to the reference" in str(w.message) for w in caught)
        assert np.array_equal(got, ref_idw(xy, uv, xg, yg, **kw), equal_nan=True)
    frames = rng.random((2, 64, 64)).astype(np.float32)
    for bad in (dict(fd_kwargs={"block_size": 4}), dict(fd_kwargs={"block_size": 9}), dict(lk_kwargs={"winsize": (80, 80)}),
                dict(interp_kwargs={"k": 50})):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            # the reference takes the call; here it stops at its own first line: OpenCV is not installed
            with pytest.raises(MissingOptionalDependency):
                dense_lucaskanade(frames, **bad)
        assert any("delegating to the reference" in str(w.message) for w in caught)
