"""tests/helpers/idw_exact.py, the exact tie-aware IDW yardstick of tests/test_idw_ties_gpu.py, held on the CPU:
it agrees with the cKDTree oracle where there is no tie, accepts every r-subset of a tie set, and rejects a member
too few, a member too many and a farther sample in a nearer one's place."""

import numpy as np
import pytest

from helpers import idw_exact
from oracle import sparse as osp


def _inputs(seed=5, L=148, m=64, n=64):
    rng = np.random.default_rng(seed)
    cells = rng.permutation(m * n)[:L]
    xy = np.column_stack([cells % n, cells // n]).astype(np.float64)
    uv = rng.normal(0.0, 2.0, (L, 2)).astype(np.float32).astype(np.float64)
    return xy, uv, np.arange(n, dtype=np.float64), np.arange(m, dtype=np.float64)


@pytest.fixture(scope="module", params=[5, 20])
def exact(request):
    xy, uv, xg, yg = _inputs()
    return idw_exact.IdwExact(xy, uv, xg, yg, k=request.param)


def _passes(ex, field):
    near = ex.nearest_valid(field)
    bad, _ = ex.invalid(field)
    den = np.linalg.norm(near)
    return bad == 0 and np.max(np.abs(field - near)) <= idw_exact.MAX_ABS and \
        np.linalg.norm(field - near) / den < idw_exact.REL_L2


def _selection_field(ex, sel):
    return idw_exact.field_from_selection(ex.xy, ex.uv, np.arange(ex.n), np.arange(ex.m), sel, ex.power, ex.dist_offset)


def test_inputs_are_exact_and_have_ties(exact):
    xy, _, xg, yg = _inputs()
    assert idw_exact.squared_distances_exact(xy, xg, yg)
    assert not idw_exact.squared_distances_exact(xy + 0.1, xg, yg)  # 0.1 is no float32 number
    assert exact.n_tie > 0.05 * exact.m * exact.n and exact.largest_group >= 3
    assert exact.discriminating() >= 100
    assert exact.on_node == len(xy)


def test_rule_field_matches_ckdtree_oracle_off_ties(exact):
    want = osp.idw(exact.xy, exact.uv, exact.m, exact.n, k=exact.k)
    keep = ~exact.tie_mask
    assert keep.sum() > 0.5 * keep.size
    assert np.max(np.abs(exact.field - want)[:, keep]) <= 1e-12
    # the selection written out sample by sample gives the same field everywhere
    again = _selection_field(exact, exact.order[:, :exact.k])
    assert np.max(np.abs(again - exact.field)) <= 1e-12


def test_all_samples_have_no_ties():
    xy, uv, xg, yg = _inputs(L=30)
    for k in (None, 30, 45):
        ex = idw_exact.IdwExact(xy, uv, xg, yg, k=k)
        assert ex.k == 30 and ex.n_tie == 0 and ex.candidates() == []
        assert np.max(np.abs(ex.field - osp.idw(xy, uv, ex.m, ex.n, k=k))) <= 1e-12


def test_scaled_grid_power_and_offset():
    """res = mean grid spacing; power and offset as given (the reference formula, written out per node)."""
    xy, uv, _, _ = _inputs(L=40, m=30, n=50)
    xg, yg = np.arange(0, 100, 2.0), np.arange(0, 60, 4.0)
    ex = idw_exact.IdwExact(2.0 * xy, uv, xg, yg, k=7, power=2.0, dist_offset=0.1)
    assert ex.res == 3.0
    row, col = 3, 11
    d = np.hypot(2.0 * xy[:, 0] - xg[col], 2.0 * xy[:, 1] - yg[row])
    o = np.argsort(d, kind="stable")[:7]
    w = 1.0 / (d[o] / 3.0 + 0.1) ** 2.0
    assert np.allclose(ex.field[:, row, col], (w[:, None] * uv[o]).sum(axis=0) / w.sum(), rtol=1e-13, atol=0)


def test_accepts_the_rule_and_any_other_subset(exact):
    assert _passes(exact, exact.field)
    assert exact.off_rule(exact.field)[0] == 0
    # the HIGHEST-index members of every tie set instead of the lowest: valid, but not the rule
    sel = []
    for p in range(exact.m * exact.n):
        ns, nt, r = int(exact.n_less[p]), int(exact.n_equal[p]), int(exact.r[p])
        sel.append(list(exact.order[p, :ns]) + list(exact.order[p, ns + nt - r:ns + nt]))
    other = _selection_field(exact, sel)
    assert _passes(exact, other)
    bad, text = exact.off_rule(other)
    assert bad >= 100 and "S=" in text and "T=" in text  # the rule check tells them apart, and says where


def _wrong_count_at_ties(exact, count):
    """the rule's field, but with ``count`` members at the tie pixels (every other pixel is right)"""
    sel = [list(row) for row in exact.order[:, :exact.k]]
    for p in np.flatnonzero(exact.tie):
        sel[p] = list(exact.order[p, :count])
    return _selection_field(exact, sel)


def test_rejects_k_minus_one_members(exact):
    field = _wrong_count_at_ties(exact, exact.k - 1)
    assert not _passes(exact, field)
    assert exact.invalid(field)[0] > 0.9 * exact.n_tie


def test_rejects_k_plus_one_members(exact):
    field = _wrong_count_at_ties(exact, exact.k + 1)
    assert not _passes(exact, field)
    assert exact.invalid(field)[0] > 0.9 * exact.n_tie


def test_rejects_a_farther_sample_in_place_of_a_member(exact):
    """the first sample beyond S and T (strictly farther than the k-th) for the nearest one, on tie pixels only:
    everything else about those pixels is right"""
    sel = [list(row) for row in exact.order[:, :exact.k]]
    swapped = 0
    for p in np.flatnonzero(exact.tie):
        beyond = int(exact.n_less[p] + exact.n_equal[p])
        if exact.n_less[p] > 0:
            sel[p][0] = int(exact.order[p, beyond])
            swapped += 1
    assert swapped >= 100
    field = _selection_field(exact, sel)
    assert not _passes(exact, field)
    bad, text = exact.invalid(field)
    assert bad > 0.9 * swapped and "r=" in text


def test_subset_cap_is_asserted():
    """a ring of 14 samples equidistant from one node, k = 7: C(14, 7) = 3432 subsets"""
    ring = [(5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (3, -4), (-3, 4), (-3, -4), (4, 3), (4, -3), (-4, 3), (-4, -3)]
    big = [(25 * x // 5, 25 * y // 5) for x, y in ring] + [(7, 24), (24, 7)]  # all at squared distance 625
    xy = np.array(big, dtype=np.float64) + 30.0
    uv = np.random.default_rng(1).normal(0, 2, xy.shape)
    ex = idw_exact.IdwExact(xy, uv, np.array([30.0]), np.array([30.0]), k=7)
    assert ex.n_tie == 1 and ex.largest_group == 14
    with pytest.raises(AssertionError):
        ex.candidates()
