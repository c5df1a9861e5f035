"""rbfinterp2d on the device (csrc/rbf.hip) against the reference's own function.

Reference: pysteps/utils/interpolate.py:117-170 (a wrapper of scipy.interpolate.Rbf) behind the preamble
of pysteps/decorators.py:153-250, imported from oracle/_ref.  The weights here are SciPy's own solve (the same
call the reference makes), the device evaluates  sum_j w_j phi(|x - x_j|)  in float64: the two results
differ by the order of a float64 sum whose terms alternate in sign - bar: relative L2 <= 1e-9, observed
values in gpurun_out/rbf_seen.json.  Mirrors pysteps/tests/test_utils_interpolate.py: shapes, finiteness,
single sample / uniform values -> uniform field, error cases.

That norm is blind to a handful of wrong pixels and depends on the conditioning of the system, so the kernel is also
held pixel by pixel to the longdouble oracle of tests/helpers/rbf.py, ``|got - S| <= (N + 16) 2^-53 B`` (derived there),
through the entry point on the fixed case list and through the wrapper; the worst ratios go to rbf_seen.json too."""

import json
import os
import warnings

import numpy as np
import pytest

from conftest import rel_l2
from helpers import rbf as H

pytestmark = pytest.mark.gpu

SEEN = []


@pytest.fixture(scope="module")
def rbf():
    from pysteps_amd.utils import rbfinterp2d

    yield rbfinterp2d
    try:
        os.makedirs("gpurun_out", exist_ok=True)
        with open("gpurun_out/rbf_seen.json", "w") as fh:
            json.dump(SEEN, fh)
    except OSError:
        pass


def _samples(n_samples, shape, seed, nvar=2):
    rng = np.random.default_rng(seed)
    m, n = shape
    # declustered-like positions: one sample per cell of a coarse lattice, jittered
    side = int(np.ceil(np.sqrt(n_samples)))
    cells = rng.permutation(side * side)[:n_samples]
    cy, cx = np.divmod(cells, side)
    xy = np.column_stack([(cx + rng.random(n_samples)) * (n - 1) / side, (cy + rng.random(n_samples)) * (m - 1) / side])
    values = rng.normal(0.0, 2.0, (n_samples, nvar)) + np.array([2.0, -1.0, 0.5][:nvar])
    return xy, values if nvar > 1 else values[:, 0]


@pytest.mark.parametrize("function", ["multiquadric", "inverse", "gaussian", "linear", "cubic", "quintic", "thin_plate"])
def test_every_basis_function_matches_the_reference(rbf, ref_pysteps, function):
    from pysteps.utils.interpolate import rbfinterp2d as ref

    shape = (97, 131)
    xy, values = _samples(60, shape, seed=len(function))
    xgrid, ygrid = np.arange(shape[1], dtype=float), np.arange(shape[0], dtype=float)
    want = ref(xy, values, xgrid, ygrid, function=function)
    got = rbf(xy, values, xgrid, ygrid, function=function)
    assert got.shape == want.shape == (2,) + shape and got.dtype == np.float64 and np.isfinite(got).all()
    err = rel_l2(got, want)
    SEEN.append((function, err))
    assert err <= 1e-9, err


@pytest.mark.parametrize("nvar,n_samples,kwargs", [(2, 40, {}), (2, 300, {"epsilon": 7.5}), (3, 80, {"smooth": 0.1}),
                                                   (2, 50, {"function": "gaussian", "epsilon": 30.0, "nchunks": 9})])
def test_variables_options_and_grids(rbf, ref_pysteps, nvar, n_samples, kwargs):
    from pysteps.utils.interpolate import rbfinterp2d as ref

    shape = (64, 200)
    xy, values = _samples(n_samples, shape, seed=n_samples, nvar=nvar)
    xgrid, ygrid = np.linspace(-3.0, 250.0, shape[1]), np.linspace(10.0, 80.0, shape[0])  # any regular grid
    want = ref(xy, values, xgrid, ygrid, **kwargs)
    got = rbf(xy, values, xgrid, ygrid, **kwargs)
    assert got.shape == want.shape
    err = rel_l2(got, want)
    SEEN.append(("nvar%d n%d %s" % (nvar, n_samples, sorted(kwargs)), err))
    assert err <= 1e-9, err


def test_trivial_cases_errors_and_delegation(rbf, ref_pysteps):
    from pysteps.utils.interpolate import rbfinterp2d as ref

    xgrid, ygrid = np.arange(20.0), np.arange(12.0)
    one = rbf(np.array([[3.0, 4.0]]), np.array([[1.5, -2.0]]), xgrid, ygrid)  # decorators.py:200-203
    assert one.shape == (2, 12, 20) and np.all(one[0] == 1.5) and np.all(one[1] == -2.0)
    same = rbf(np.array([[3.0, 4.0], [7.0, 1.0]]), np.array([2.0, 2.0]), xgrid, ygrid)  # :207-208
    assert same.shape == (1, 12, 20) and np.all(same == 2.0)  # (no squeeze in that branch of the reference either)
    xy, values = _samples(20, (12, 20), seed=3)
    bad = values.copy()
    bad[2, 0] = np.nan
    with pytest.raises(ValueError):
        rbf(xy, bad, xgrid, ygrid)
    with pytest.raises(ValueError):
        rbf(xy, values[:-1], xgrid, ygrid)
    with pytest.warns(DeprecationWarning):
        assert rel_l2(rbf(xy, values, xgrid, ygrid, rbfunction="gaussian"), ref(xy, values, xgrid, ygrid, rbfunction="gaussian")) <= 1e-9
    # 1-d values: the reference's own axis handling (a transposition per grid chunk, interpolate.py:169) applies
    with pytest.warns(UserWarning, match="delegating"):
        got = rbf(xy, values[:, 0], np.arange(12.0), ygrid)
    assert np.array_equal(got, ref(xy, values[:, 0], np.arange(12.0), ygrid))
    # a callable basis function and an irregular grid are the reference's job (delegated with a warning)
    irregular = np.array(sorted(np.random.default_rng(0).random(20) * 19.0))
    with pytest.warns(UserWarning, match="delegating"):
        got = rbf(xy, values, irregular, ygrid)
    assert np.allclose(got, ref(xy, values, irregular, ygrid))
    with pytest.warns(UserWarning, match="delegating"):
        got = rbf(xy, values, xgrid, ygrid, function=lambda self, r: r ** 2 + 1.0)
    assert got.shape == (2, 12, 20)


def test_full_size_grid_runs_and_interpolates(rbf):
    """4096 x 4096 with 900 vectors (what dense_lucaskanade hands over after declustering): the interpolant
    goes through its samples."""
    m = n = 4096
    xy, values = _samples(900, (m, n), seed=11)
    xy = np.round(xy)  # on grid nodes, so that the samples can be read back
    _, keep = np.unique(xy, axis=0, return_index=True)
    xy, values = xy[keep], values[keep]
    got = rbf(xy, values, np.arange(n), np.arange(m))
    assert got.shape == (2, m, n) and np.isfinite(got).all()
    back = got[:, xy[:, 1].astype(int), xy[:, 0].astype(int)].T
    assert np.abs(back - values).max() <= 1e-6 * np.abs(values).max()
    # 4096 seeded pixels of those planes against the oracle (no further device work): the corners, the last row and the
    # last column among them, beyond the first 2^24 elements of a plane and in both planes
    rbfi = H.solve(xy, values, "multiquadric")
    rng = np.random.default_rng(4096)
    iy, ix = rng.integers(0, m, 4096), rng.integers(0, n, 4096)
    iy[:6], ix[:6] = [0, 0, m - 1, m - 1, m - 1, 1234], [0, n - 1, 0, n - 1, 2345, n - 1]
    geometry = (m, n, 0.0, 1.0, 0.0, 1.0)
    S, B = H.oracle(xy, rbfi.nodes, len(xy), *geometry, "multiquadric", rbfi.epsilon, pixels=(iy, ix))
    Bar = H.bar(xy, rbfi.nodes, len(xy), *geometry, "multiquadric", rbfi.epsilon, B, pixels=(iy, ix))
    ratio, at = H.check(got[:, iy, ix], S, Bar)
    SEEN.append(("full-size", "multiquadric", len(xy), ratio * (len(xy) + H.PHI_COST), ratio))
    assert ratio <= 1.0, (ratio, at, iy[at[1]], ix[at[1]])


# ---- every pixel against the wide oracle -------------------------------------------------------------------------------

def _entry(xy, w, geometry, function, epsilon):
    """psh_rbf_eval_dev itself, on a buffer of NaN: ``(2, m, n)``."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    m, n, x0, dx, y0, dy = geometry
    xy, w = np.ascontiguousarray(xy, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
    assert xy.shape == w.shape and xy.shape[1] == 2
    xy_d, w_d = DeviceArray.from_host(xy), DeviceArray.from_host(w)
    out = DeviceArray.from_host(np.full((2, m, n), np.nan))
    _lib.check(_lib.lib().psh_rbf_eval_dev(xy_d.ptr, w_d.ptr, xy.shape[0], m, n, x0, dx, y0, dy, H.CODE[function],
                                           float(epsilon), out.ptr), "psh_rbf_eval_dev")
    return np.array(out.to_host())


@pytest.mark.parametrize("function", H.FUNCTIONS)
def test_every_pixel_is_within_the_bar_of_the_oracle(rbf, function):
    failed = []
    for c in H.cases(function):
        S, Bar, _ = c.yardstick()
        got = _entry(c.xy, c.w, c.geometry(), function, c.epsilon)
        ratio, at = H.check(got, S, Bar)
        SEEN.append((c.name, function, c.N, ratio * (c.N + H.PHI_COST), ratio))
        print("%s %s N=%d: worst %.3f of the bar (%.2f units of 2^-53 B) at %s" % (function, c.name, c.N, ratio, ratio * (c.N + H.PHI_COST), at))
        if not (ratio <= 1.0 and np.isfinite(got).all()):
            failed.append((c.name, ratio, at))
        if c.on_nodes:  # smooth = 0: the interpolant goes through its samples, within the same bar
            iy, ix = c.node_pixels()
            if not np.all(np.abs(got[:, iy, ix].T.astype(H.LD) - c.values) <= Bar[:, iy, ix].T):
                failed.append((c.name, "samples not reproduced"))
        if c.name == "zero-second" and not np.all(got[1] == 0.0):
            failed.append((c.name, "plane 1 is not exactly zero"))
        if c.name == "on-nodes-eps0.05":  # w_j at the nodes; nothing where every term underflows (r >= 2: exp(-1600))
            iy, ix = c.node_pixels()
            far = np.ones((c.m, c.n), dtype=bool)
            for sy in (-1, 0, 1):
                for sx in (-1, 0, 1):
                    far[np.clip(iy + sy, 0, c.m - 1), np.clip(ix + sx, 0, c.n - 1)] = False
            if not (np.array_equal(got[:, iy, ix].T, c.w) and np.all(got[:, far] == 0.0)):
                failed.append((c.name, "not w_j at the nodes and zero elsewhere"))
    assert not failed, failed


@pytest.mark.parametrize("nvar,kwargs", [(3, {}), (2, {"smooth": 0.1}), (1, {}), (3, {"function": "thin_plate", "smooth": 0.1})])
def test_wrapper_hands_the_kernel_scipys_weights(rbf, nvar, kwargs):
    """Through rbfinterp2d: bit for bit the entry point called with ``Rbf(...).nodes`` and ``Rbf(...).epsilon`` (three
    variables: two launches, the second padded with a zero column; one variable given as (N, 1)), and within the bar
    of the oracle evaluated with those weights."""
    from scipy.interpolate import Rbf

    m, n, N = 33, 70, 80
    function = kwargs.get("function", "multiquadric")
    rng = np.random.default_rng([nvar, len(kwargs)])
    xy = H._jittered(N, n - 1, m - 1, rng)
    values = rng.normal(0.0, 2.0, (N, nvar)) + np.array([2.0, -1.0, 0.5][:nvar])
    geometry = (m, n, -3.25, 0.75, 10.5, -0.5)  # exactly representable, descending y
    xgrid, ygrid = -3.25 + 0.75 * np.arange(n), 10.5 - 0.5 * np.arange(m)
    xy = np.column_stack([-3.25 + 0.75 * xy[:, 0], 10.5 - 0.5 * xy[:, 1]])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = rbf(xy, values, xgrid, ygrid, **kwargs)
    assert not [w for w in seen if "delegating" in str(w.message)]
    assert got.shape == ((nvar, m, n) if nvar > 1 else (m, n))
    got = got.reshape(nvar, m, n)
    rbfi = Rbf(xy[:, 0], xy[:, 1], values, mode="N-D", **kwargs)
    nodes = np.asarray(rbfi.nodes).reshape(N, nvar)
    for c0 in range(0, nvar, 2):
        width = min(2, nvar - c0)
        pair = np.zeros((N, 2))
        pair[:, :width] = nodes[:, c0:c0 + width]
        direct = _entry(xy, pair, geometry, function, rbfi.epsilon)
        assert np.array_equal(got[c0:c0 + width], direct[:width])
        if width == 1:
            assert np.all(direct[1] == 0.0)
        S, B = H.oracle(xy, pair, N, *geometry, function, rbfi.epsilon)
        ratio, at = H.check(direct, S, H.bar(xy, pair, N, *geometry, function, rbfi.epsilon, B))
        SEEN.append(("wrapper nvar%d %s cols %d.." % (nvar, sorted(kwargs.items()), c0), function, N, ratio * (N + H.PHI_COST), ratio))
        assert ratio <= 1.0, (ratio, at)


def drifting_axis(n=200):
    """Steps that are all 9e-10 longer than the first: ``np.allclose(steps, steps[0], rtol=1e-9)`` calls it regular."""
    i = np.arange(n)
    return i + 9e-10 * np.maximum(i - 1, 0)


def test_a_drifting_grid_is_evaluated_where_it_was_given(rbf, ref_pysteps):
    """The result belongs to the xgrid positions as given, not to ``x0 + dx i`` with the first step for dx: by column
    199 the two are 1.8e-7 apart, a cubic interpolant moves by over a hundred bars on the way there (138 measured
    with the former ``np.allclose(steps, steps[0], rtol=1e-9)`` criterion, at column 70)."""
    m, n, N = 20, 200, 60
    rng = np.random.default_rng(5)
    xy, values = H._jittered(N, n - 1, m - 1, rng), H._values(N, rng)
    xgrid, ygrid = drifting_axis(n), np.arange(m, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (whichever path takes the call)
        got = rbf(xy, values, xgrid, ygrid, function="cubic")
    rbfi = H.solve(xy, values, "cubic")
    S, Bar = np.empty((2, m, n), dtype=H.LD), np.empty((2, m, n), dtype=H.LD)
    for ix in range(n):  # the oracle at the given positions, a column at a time
        geometry = (m, 1, float(xgrid[ix]), 1.0, 0.0, 1.0)
        s, b = H.oracle(xy, rbfi.nodes, N, *geometry, "cubic", rbfi.epsilon)
        S[:, :, ix], Bar[:, :, ix] = s[:, :, 0], H.bar(xy, rbfi.nodes, N, *geometry, "cubic", rbfi.epsilon, b)[:, :, 0]
    ratio, at = H.check(got, S, Bar)
    SEEN.append(("drifting-grid", "cubic", N, ratio * (N + H.PHI_COST), ratio))
    assert ratio <= 1.0, (ratio, at)


def test_regular_grids_of_the_suite_reach_the_device(rbf):
    """arange, linspace, scaled and shifted axes: none of them is sent to the reference."""
    from pysteps_amd.utils import idwinterp2d

    rng = np.random.default_rng(8)
    grids = [(np.arange(131), np.arange(97)), (np.arange(131, dtype=float), np.arange(97, dtype=float)),
             (np.linspace(-3.0, 250.0, 200), np.linspace(10.0, 80.0, 64)), (np.arange(0, 100, 2.0), np.arange(0, 60, 2.0)),
             (np.arange(5, 35) * 2.0, np.arange(20) * 2.0), (np.arange(30), np.arange(20)), (np.arange(0, 100, 2.0), np.arange(0, 60, 4.0)),
             (255000.0 + 1000.0 * np.arange(65), 500000.0 - 1000.0 * np.arange(33))]
    for xgrid, ygrid in grids:
        xy = np.column_stack([rng.uniform(xgrid.min(), xgrid.max(), 25), rng.uniform(ygrid.min(), ygrid.max(), 25)])
        values = rng.normal(size=(25, 2))
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            a = rbf(xy, values, xgrid, ygrid)
            b = idwinterp2d(xy, values, xgrid, ygrid)
        assert not [w for w in seen if "delegating" in str(w.message)], (xgrid[:3], [str(w.message) for w in seen])
        assert a.shape == b.shape == (2, ygrid.size, xgrid.size) and np.isfinite(a).all() and np.isfinite(b).all()
