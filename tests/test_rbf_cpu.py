"""tests/helpers/rbf.py, the pointwise yardstick of tests/test_rbf_gpu.py, held on the CPU.

* The inputs leave honest float64 evaluations well inside the bar: the NumPy model of the kernel, summed forward,
  reversed and pairwise, stays below a quarter of it ((N + 16) / 4 units of 2^-53 B) on every case of every function;
  SciPy's own ``Rbf.__call__`` passes on the cases whose weights are its solve.
* The check is sharp: each seeded defect of ``emulate`` - the mistakes the kernel's seams invite - is rejected on a
  named case, so that a later trimming of the case list cannot quietly lose the coverage.
* The longdouble oracle agrees with mpmath at 50 digits to 2^-60 B.
* ``_regular_axis`` accepts the grids the kernel can reproduce and no others.
"""

import warnings

import numpy as np
import pytest

from helpers import rbf as H


@pytest.mark.parametrize("function", H.FUNCTIONS)
def test_honest_evaluations_stay_inside_a_quarter_of_the_bar(function):
    worst = (0.0, None)
    for c in H.cases(function):
        S, Bar, _ = c.yardstick()
        for order in H.ORDERS:
            got = H.emulate(c, order)
            ratio, at = H.check(got, S, Bar)
            worst = max(worst, (ratio * (c.N + H.PHI_COST), "%s %s N=%d at %s" % (c.name, order, c.N, at)))
            assert ratio < 0.25, (c.name, order, ratio * (c.N + H.PHI_COST), at)  # < (N + 16) / 4 units of u B
            if c.on_nodes:  # smooth = 0: the interpolant goes through its samples
                iy, ix = c.node_pixels()
                assert np.all(np.abs(got[:, iy, ix].T.astype(H.LD) - c.values) <= Bar[:, iy, ix].T), (c.name, order)
    print("%s: worst honest evaluation %.2f units of 2^-53 B (%s)" % (function, *worst))


@pytest.mark.parametrize("function", H.FUNCTIONS)
def test_scipy_call_passes_where_the_weights_are_its_solve(function):
    solved = [c for c in H.cases(function) if c.rbfi is not None]
    assert len(solved) >= 14
    worst = 0.0
    for c in solved:
        S, Bar, _ = c.yardstick()
        ratio, at = H.check(H.scipy_eval(c), S, Bar)
        worst = max(worst, ratio * (c.N + H.PHI_COST))
        assert ratio <= 1.0, (c.name, ratio, at)
    print("%s: worst SciPy evaluation %.2f units of 2^-53 B" % (function, worst))


def test_case_list_covers_the_seams():
    for function in H.FUNCTIONS:
        cs = {c.name: c for c in H.cases(function)}
        assert {(c.m, c.n) for c in cs.values() if c.name.startswith("tile-edges")} == {(17, 65), (15, 63), (16, 64)}
        assert {(cs[k].m, cs[k].n, cs[k].N) for k in ("thin-1x130", "thin-33x1", "thin-1x1")} == {(1, 130, 3), (33, 1, 3), (1, 1, 3)}
        assert [cs["chunk-N%d" % N].N for N in (255, 256, 257, 513)] == [255, 256, 257, 513]
        on = cs["on-nodes"]
        assert 280 <= on.N <= 300 and on.N > H.CHUNK and len(on.node_pixels()[0]) == on.N
        out = cs["outside"]
        beyond = (out.xy[:, 0] < 0) | (out.xy[:, 0] > 69) | (out.xy[:, 1] < 0) | (out.xy[:, 1] > 19)
        assert beyond.sum() == 20 and np.abs(out.xy[:, 0]).max() > 69
        assert cs["metres"].dy == -1000.0 and cs["metres"].N % H.CHUNK == 1
        assert cs["inexact"].coordinate and not any(c.coordinate for k, c in cs.items() if k != "inexact")
        for c in cs.values():  # the strict cases: exactly representable pixel coordinates (products and sums exact)
            if not c.coordinate:
                for o, d, k in ((c.x0, c.dx, c.n), (c.y0, c.dy, c.m)):
                    i = np.arange(k)
                    assert np.array_equal((o + d * i).astype(H.LD), H.LD(o) + H.LD(d) * i.astype(H.LD)), c.name
        assert not cs["zero-second"].w[:, 1].any() and cs["zero-second"].w[:, 0].all()
        w = np.abs(cs["dynamic-range"].w)
        assert w.max() == 1e12 and np.sort(w, axis=0)[-2].max() < 10.0
        has_eps = function in H.EPSILON_BEARING
        assert ("tile-edges-17x65-eps0.001" in cs) == has_eps and ("tile-edges-17x65-eps1e+06" in cs) == has_eps
        assert ("on-nodes-eps0.05" in cs) == (function == "gaussian")


def test_zero_weights_and_underflow_are_exact_in_the_oracle():
    for function in H.FUNCTIONS:
        S, Bar, _ = H.case(function, "zero-second").yardstick()
        assert np.all(S[1] == 0) and np.all(Bar[1] == 0) and np.all(Bar[0] > 0)
    c = H.case("gaussian", "on-nodes-eps0.05")
    assert np.array_equal(c.w, c.values)  # the system is the identity
    got = H.emulate(c)
    iy, ix = c.node_pixels()
    assert np.array_equal(got[:, iy, ix].T, c.w)
    far = np.ones((c.m, c.n), dtype=bool)
    for sy in (-1, 0, 1):
        for sx in (-1, 0, 1):
            far[np.clip(iy + sy, 0, c.m - 1), np.clip(ix + sx, 0, c.n - 1)] = False
    assert far.sum() > 100 and np.all(got[:, far] == 0.0)  # r >= 2: exp(-1600) is no float64 number


# defect -> (function, case) it must be rejected on; (function, case) it must leave alone
REJECTED = {
    "drop_chunk_tail": [(f, "chunk-N257") for f in H.FUNCTIONS] + [("cubic", "metres"), ("linear", "chunk-N513")],
    "row_stride": [(f, "tile-edges-17x65") for f in H.FUNCTIONS] + [("multiquadric", "thin-33x1"), ("gaussian", "metres")],
    "second_var_reads_first": [(f, "tile-edges-16x64") for f in H.FUNCTIONS] + [("inverse", "zero-second")],
    "phi_float32": [(f, "tile-edges-15x63") for f in H.FUNCTIONS] + [("quintic", "dynamic-range")],
    "thin_plate_nan_at_zero": [("thin_plate", "on-nodes")],
    "last_column_stale": [(f, "tile-edges-17x65") for f in H.FUNCTIONS] + [("thin_plate", "chunk-N256"), ("linear", "thin-33x1")],
    "gaussian_eps_not_squared": [("gaussian", "tile-edges-17x65"), ("gaussian", "tile-edges-16x64-eps0.001"),
                                 ("gaussian", "on-nodes-eps0.05")],
}
UNTOUCHED = {
    "drop_chunk_tail": [("cubic", "chunk-N256"), ("cubic", "chunk-N255")],
    "thin_plate_nan_at_zero": [("thin_plate", "tile-edges-17x65"), ("cubic", "on-nodes")],
    "last_column_stale": [("linear", "tile-edges-16x64")],
    "gaussian_eps_not_squared": [("multiquadric", "tile-edges-17x65")],
}


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_every_seeded_defect_is_rejected_on_a_named_case(defect):
    assert REJECTED[defect]
    for function, name in REJECTED[defect]:
        c = H.case(function, name)
        S, Bar, _ = c.yardstick()
        assert H.check(H.emulate(c), S, Bar)[0] < 0.25
        ratio, at = H.check(H.emulate(c, defect=defect), S, Bar)
        assert ratio > 1.0, (defect, function, name, ratio)
    for function, name in UNTOUCHED.get(defect, []):
        c = H.case(function, name)
        assert np.array_equal(H.emulate(c, defect=defect), H.emulate(c)), (defect, function, name)


def test_a_single_wrong_pixel_is_seen_where_a_norm_is_blind():
    """One pixel of the last tile row off by a part in 1e12 of its unit: nothing to a relative L2 over the plane."""
    from conftest import rel_l2

    c = H.case("multiquadric", "tile-edges-17x65")
    S, Bar, B = c.yardstick()
    got = H.emulate(c)
    got[1, 16, 64] += 1e-12 * float(B[1, 16, 64])
    assert rel_l2(got, S.astype(np.float64)) < 1e-9
    ratio, at = H.check(got, S, Bar)
    assert ratio > 1.0 and at == (1, 16, 64)
    nan = H.emulate(c)
    nan[0, 3, 5] = np.nan
    assert H.check(nan, S, Bar) == (np.inf, (0, 3, 5))


def test_longdouble_oracle_agrees_with_mpmath():
    """200 (function, case, pixel) triples, every function and the corners among them, to 2^-60 B."""
    import mpmath

    rng = np.random.default_rng(2024)
    mp = mpmath.mp.clone()
    mp.dps = 50
    names = ("tile-edges-17x65", "thin-1x130", "chunk-N257", "on-nodes", "outside", "metres", "dyadic", "inexact", "dynamic-range")
    picks = [(H.FUNCTIONS[i % 7], names[i % len(names)]) for i in range(200)]
    picks[:3] = [("gaussian", "on-nodes-eps0.05"), ("gaussian", "tile-edges-17x65-eps0.001"), ("multiquadric", "tile-edges-16x64-eps1e+06")]
    by_case = {}
    for i, key in enumerate(picks):
        c = H.case(*key)
        if c.on_nodes and i % 2 == 0:  # a pixel that is a node: r2 = 0 among the terms
            iy, ix = (int(a[i % c.N]) for a in c.node_pixels())
        else:
            iy, ix = [(0, 0), (0, c.n - 1), (c.m - 1, 0), (c.m - 1, c.n - 1), (int(rng.integers(c.m)), int(rng.integers(c.n)))][min(i % 9, 4)]
        by_case.setdefault(key, []).append((iy, ix))
    worst = 0.0
    for key, pix in by_case.items():
        c = H.case(*key)
        S, _, B = c.yardstick()
        iy, ix = np.array(pix).T
        Sm, Bm = H.oracle_mp(c.xy, c.w, *c.geometry(), c.function, c.epsilon, (iy, ix))
        for k in range(2):
            # longdouble's own underflow (a Gaussian term below 2^-16382): an absolute 2^-16382 per unit of weight
            under = mp.mpf(float(np.abs(c.w[:, k]).sum())) * mp.mpf(2) ** -16382
            for p, (y, x) in enumerate(pix):
                err = abs(H._ld_to_mp(mp, S[k, y, x]) - Sm[k][p])
                assert err <= Bm[k][p] * mp.mpf(2) ** -60 + under, (key, k, y, x, float(err / Bm[k][p]))
                assert abs(H._ld_to_mp(mp, B[k, y, x]) - Bm[k][p]) <= Bm[k][p] * mp.mpf(2) ** -55 + under
                if Bm[k][p] > under * mp.mpf(2) ** 64:
                    worst = max(worst, float(err / Bm[k][p]))
    assert sum(len(v) for v in by_case.values()) == 200
    print("longdouble oracle vs mpmath: worst %.2f x 2^-64 B" % (worst * 2.0 ** 64))


# ---- the grid the wrapper accepts --------------------------------------------------------------------------------------

def drifting_axis(n=200):
    """Steps that are all 9e-10 longer than the first: ``np.allclose(steps, steps[0], rtol=1e-9)`` calls it regular."""
    i = np.arange(n)
    return i + 9e-10 * np.maximum(i - 1, 0)


def test_regular_axis_accepts_what_the_kernel_reproduces_and_nothing_else():
    from pysteps_amd.utils.interpolate import _regular_axis

    drift = drifting_axis()
    steps = np.diff(drift)
    assert np.allclose(steps, steps[0], rtol=1e-9, atol=0.0) and abs(drift[-1] - 199.0) > 1.7e-7
    assert _regular_axis(drift, "xgrid") is None
    assert _regular_axis(drift[::-1], "xgrid") is None
    regular = [np.arange(131), np.arange(4096), np.arange(97.0), np.linspace(-3.0, 250.0, 200), np.linspace(10.0, 80.0, 64),
               np.arange(0, 100, 2.0), np.arange(0, 60, 2.0), np.arange(0, 60, 4.0), np.arange(5, 35) * 2.0, np.arange(20) * 2.0,
               np.arange(26, 38), 255000.0 + 1000.0 * np.arange(65), 500000.0 - 1000.0 * np.arange(33), -3.25 + 0.75 * np.arange(70),
               np.linspace(0.0, 1.0, 4096), np.linspace(-1e6, 1e6, 777), np.arange(0.0, 30.0, 0.1), np.array([2.0, 5.0])]
    for g in regular:
        origin, spacing = _regular_axis(g, "xgrid")
        assert origin == g[0] and np.max(np.abs(origin + spacing * np.arange(g.size) - g)) <= 4 * np.spacing(np.abs(g).max())
        if np.array_equal(g, np.round(g)):
            assert spacing == g[1] - g[0]
    assert _regular_axis(np.array([7.5]), "xgrid") == (7.5, 1.0)
    for g in (np.array([0.0, 1.0, 2.0, 3.5]), np.array([1.0, 1.0, 1.0]), np.array([0.0, 0.0, 2.0]), np.array([0.0, 1.0, 2.0 + 1e-12]),
              np.sort(np.random.default_rng(0).random(20) * 19.0)):
        assert _regular_axis(g, "xgrid") is None
    with pytest.raises(ValueError):
        _regular_axis(np.zeros((2, 2)), "xgrid")
    with pytest.raises(ValueError):
        _regular_axis(np.array([]), "xgrid")


def test_drifting_axis_is_off_by_far_more_than_the_bar():
    """The arithmetic behind the criterion: evaluated on ``x0 + dx i`` with the first step for dx, the cubic
    interpolant is off the one at the given positions by thousands of bars at the last column."""
    c = H.case("cubic", "tile-edges-17x65")
    xg = drifting_axis(c.n)
    S, Bar, _ = c.yardstick()
    given = np.empty((2, c.m, c.n), dtype=H.LD)
    for ix in range(c.n):  # the oracle at the given positions, a column at a time
        col, _ = H.oracle(c.xy, c.w, c.N, c.m, 1, float(xg[ix]), 1.0, c.y0, c.dy, c.function, c.epsilon)
        given[:, :, ix] = col[:, :, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ratio, at = H.check(H.emulate(c), given, Bar)
    assert ratio > 100.0 and at[2] > 32, (ratio, at)
