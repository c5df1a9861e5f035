"""Exact float64 yardstick for the k-nearest IDW interpolation at EQUIDISTANT samples (test yardstick).

``pysteps/utils/interpolate.py`` ``idwinterp2d``: for every grid node the k nearest samples, weights
``(d / res + dist_offset) ** -power`` with ``res`` the mean grid spacing, normalised, ``out = sum w * values``.
Which of several samples at exactly the k-th distance are taken is cKDTree's business there; the HIP kernels
(``csrc/idw.hip``) document a rule: the lower sample index first.  This helper is a brute force over all samples
for every node that is exact about such ties, for inputs whose squared distances ``dx*dx + dy*dy`` are exactly
representable (integer, half- and quarter-integer positions on integer nodes): then float32 and float64 agree
bit for bit on every squared distance (``squared_distances_exact`` asserts it), and so on every tie.

Per node, with ``d_k`` the k-th smallest squared distance: the mandatory set ``S = {d2 < d_k}``, the tie set
``T = {d2 == d_k}`` and ``r = k - |S|`` members of ``T`` to take.  All members of ``T`` share one weight ``w_k``,
so the denominator ``sum_S w + r w_k`` does not depend on the choice, and the valid values of the node are
``(sum_S w uv + w_k sum_C uv) / den`` over the r-subsets ``C`` of ``T``.

* ``IdwExact.field``: the documented rule, ``S`` plus the ``r`` lowest-index members of ``T`` (= the first k
  samples of a stable sort by squared distance).
* ``IdwExact.nearest_valid(got)``: per node the valid value closest to ``got`` (all r-subsets enumerated; at most
  ``MAX_SUBSETS`` per node, asserted); ``IdwExact.invalid(got)`` lists the nodes where even that one is off by more
  than the bar, with their ``S``, ``T`` and ``r``.
"""

import itertools

import numpy as np

MAX_SUBSETS = 1000  # C(12, 6) = 924: the most a full integer lattice produces (12 samples at r^2 = 25)
MAX_ABS = 1e-4  # tests/test_idw_gpu.py: float32 arithmetic against a float64 reference
REL_L2 = 1e-5


def grid_axis(grid):
    """(origin, spacing) of a regular axis; a single node has spacing 1 (pysteps_amd/utils/interpolate.py)."""
    grid = np.asarray(grid, dtype=np.float64)
    if grid.size == 1:
        return float(grid[0]), 1.0
    steps = np.diff(grid)
    assert np.all(steps == steps[0]) and steps[0] != 0
    return float(grid[0]), float(steps[0])


def _d2(xy, gx, gy, dtype):
    """(P, L) squared distances as ``dx*dx + dy*dy`` in ``dtype``, every operation rounded to it."""
    x, y = xy[:, 0].astype(dtype), xy[:, 1].astype(dtype)
    dx = x[None, :] - gx.astype(dtype)[:, None]
    dy = y[None, :] - gy.astype(dtype)[:, None]
    return dx * dx + dy * dy


def squared_distances_exact(xy, xgrid, ygrid):
    """True if positions and nodes are float32 numbers and the float32 squared distances equal the float64 ones."""
    xy = np.asarray(xy, dtype=np.float64)
    gx, gy = (a.ravel() for a in np.meshgrid(np.asarray(xgrid, np.float64), np.asarray(ygrid, np.float64)))
    if not (np.array_equal(xy.astype(np.float32), xy) and np.array_equal(gx.astype(np.float32), gx)
            and np.array_equal(gy.astype(np.float32), gy)):
        return False
    d32 = _d2(xy, gx, gy, np.float32)
    assert d32.dtype == np.float32
    return bool(np.array_equal(d32.astype(np.float64), _d2(xy, gx, gy, np.float64)))


def weights(d2, res, power, dist_offset):
    return (np.sqrt(d2) / res + dist_offset) ** (-power)


def field_from_selection(xy, uv, xgrid, ygrid, sel, power=0.5, dist_offset=0.5):
    """(2, m, n) IDW field with node p built from the samples ``sel[p]`` (a list of index lists or a (P, c) array)."""
    xy, uv = np.asarray(xy, np.float64), np.asarray(uv, np.float64)
    gx, gy = (a.ravel() for a in np.meshgrid(np.asarray(xgrid, np.float64), np.asarray(ygrid, np.float64)))
    res = 0.5 * (abs(grid_axis(xgrid)[1]) + abs(grid_axis(ygrid)[1]))
    out = np.empty((gx.size, 2))
    for p in range(gx.size):
        i = np.asarray(sel[p], dtype=np.int64)
        w = weights((xy[i, 0] - gx[p]) ** 2 + (xy[i, 1] - gy[p]) ** 2, res, power, dist_offset)
        out[p] = (w[:, None] * uv[i]).sum(axis=0) / w.sum()
    return np.moveaxis(out.reshape(np.size(ygrid), np.size(xgrid), 2), -1, 0)


class IdwExact:
    """Brute-force IDW of ``uv`` (L, 2) at the samples ``xy`` (L, 2) on the nodes ``xgrid`` x ``ygrid``."""

    def __init__(self, xy, uv, xgrid, ygrid, k=20, power=0.5, dist_offset=0.5):
        xy, uv = np.asarray(xy, np.float64), np.asarray(uv, np.float64)
        assert xy.ndim == 2 and xy.shape[1] == 2 and uv.shape == xy.shape
        assert len(np.unique(xy, axis=0)) == len(xy), "sample positions must be distinct"
        self.xy, self.uv = xy, uv
        self.m, self.n = int(np.size(ygrid)), int(np.size(xgrid))
        L = xy.shape[0]
        self.L = L
        self.k = kk = L if k is None else int(min(k, L))
        self.power, self.dist_offset = float(power), float(dist_offset)
        self.res = 0.5 * (abs(grid_axis(xgrid)[1]) + abs(grid_axis(ygrid)[1]))
        gx, gy = (a.ravel() for a in np.meshgrid(np.asarray(xgrid, np.float64), np.asarray(ygrid, np.float64)))
        P = gx.size
        # only the head of every node's sorted list is kept: S, T and the first sample beyond them
        self.keep = keep = min(L, kk + 24)
        self.order = np.empty((P, keep), dtype=np.int32)  # samples by (squared distance, index)
        self.n_less = np.empty(P, dtype=np.int64)  # |S|
        self.n_equal = np.empty(P, dtype=np.int64)  # |T|
        self.on_node = 0  # nodes that carry a sample (d = 0)
        d2s = np.empty((P, keep))  # squared distances in that order
        for p0 in range(0, P, 4096):
            p1 = min(P, p0 + 4096)
            d2 = _d2(xy, gx[p0:p1], gy[p0:p1], np.float64)
            o = np.argsort(d2, axis=1, kind="stable")
            d2 = np.take_along_axis(d2, o, axis=1)
            dk = d2[:, kk - 1:kk]
            self.order[p0:p1] = o[:, :keep]
            self.n_less[p0:p1] = (d2 < dk).sum(axis=1)
            self.n_equal[p0:p1] = (d2 == dk).sum(axis=1)
            self.on_node += int((d2[:, 0] == 0).sum())
            d2s[p0:p1] = d2[:, :keep]
        assert (self.n_less + self.n_equal).max() <= keep - (keep < L), "a tie group beyond the kept head"
        self.r = kk - self.n_less  # members of T to take, >= 1
        self.w = weights(d2s, self.res, self.power, self.dist_offset)
        assert np.isfinite(self.w).all()
        # the documented rule: a stable sort puts equal distances in index order
        wk = self.w[:, :kk]
        self.den = wk.sum(axis=1)
        self._field = (wk[..., None] * uv[self.order[:, :kk]]).sum(axis=1) / self.den[:, None]
        self.tie = self.n_less + self.n_equal > kk  # the k-th and the (k+1)-th nearest are equidistant
        self.n_tie = int(self.tie.sum())
        self.largest_group = int(self.n_equal[self.tie].max()) if self.n_tie else 0
        self._cands = None

    # ---- (a) ------------------------------------------------------------------------------------
    @property
    def field(self):
        return np.moveaxis(self._field.reshape(self.m, self.n, 2), -1, 0).copy()

    @property
    def tie_mask(self):
        return self.tie.reshape(self.m, self.n).copy()

    # ---- (b) ------------------------------------------------------------------------------------
    def candidates(self):
        """[(nodes (G,), values (G, C, 2))]: every valid value of the tie nodes, grouped by (|T|, r); the subsets
        in lexicographic order, so ``values[:, 0]`` is the documented rule's."""
        if self._cands is not None:
            return self._cands
        out = []
        tie_nodes = np.flatnonzero(self.tie)
        groups = {}
        for p in tie_nodes:
            groups.setdefault((int(self.n_equal[p]), int(self.r[p])), []).append(p)
        for (nt, r), nodes in sorted(groups.items()):
            combos = np.array(list(itertools.combinations(range(nt), r)), dtype=np.int64)  # (C, r)
            assert len(combos) <= MAX_SUBSETS, "a node with |T|=%d, r=%d needs %d subsets" % (nt, r, len(combos))
            nodes = np.asarray(nodes, dtype=np.int64)
            ns = self.n_less[nodes]
            cols = ns[:, None] + np.arange(nt)[None, :]
            t_uv = self.uv[np.take_along_axis(self.order[nodes], cols, axis=1)]  # (G, nt, 2), index order
            w_k = self.w[nodes, ns]
            in_s = np.arange(self.keep)[None, :] < ns[:, None]
            base = ((self.w[nodes] * in_s)[..., None] * self.uv[self.order[nodes]]).sum(axis=1)  # sum_S w uv
            vals = (base[:, None, :] + w_k[:, None, None] * t_uv[:, combos].sum(axis=2)) / self.den[nodes][:, None, None]
            out.append((nodes, vals))
        self._cands = out
        return out

    def discriminating(self, factor=10.0, bar=MAX_ABS):
        """tie nodes at which some other valid subset moves the value by more than ``factor * bar``."""
        count = 0
        for nodes, vals in self.candidates():
            move = np.abs(vals - vals[:, :1]).max(axis=(1, 2))
            count += int((move > factor * bar).sum())
        return count

    def nearest_valid(self, got):
        """(2, m, n): per node the valid value closest to ``got`` (largest component difference)."""
        got = np.asarray(got, np.float64)
        assert got.shape == (2, self.m, self.n)
        flat = np.moveaxis(got, 0, -1).reshape(-1, 2)
        near = self._field.copy()
        for nodes, vals in self.candidates():
            err = np.abs(vals - flat[nodes][:, None, :]).max(axis=2)  # (G, C)
            near[nodes] = vals[np.arange(len(nodes)), err.argmin(axis=1)]
        return np.moveaxis(near.reshape(self.m, self.n, 2), -1, 0)

    def describe(self, p):
        ns, nt, r = int(self.n_less[p]), int(self.n_equal[p]), int(self.r[p])
        return "node (row %d, col %d): S=%s T=%s r=%d rule %s" % (
            p // self.n, p % self.n, self.order[p, :ns].tolist(), self.order[p, ns:ns + nt].tolist(), r,
            self._field[p].tolist())

    def invalid(self, got, bar=MAX_ABS, show=5):
        """Nodes whose value matches NO valid subset within ``bar``: (count, text on the first ``show``)."""
        got = np.asarray(got, np.float64)
        err = np.abs(got - self.nearest_valid(got)).max(axis=0).ravel()
        err[~np.isfinite(err)] = np.inf
        bad = np.flatnonzero(err > bar)
        flat = np.moveaxis(got, 0, -1).reshape(-1, 2)
        lines = ["%s got %s off by %.3g" % (self.describe(p), flat[p].tolist(), err[p]) for p in bad[:show]]
        return len(bad), "\n".join(lines)

    def off_rule(self, got, bar=MAX_ABS, show=5):
        """Nodes that differ from the documented rule's field by more than ``bar``: (count, text)."""
        got = np.asarray(got, np.float64)
        err = np.abs(got - self.field).max(axis=0).ravel()
        err[~np.isfinite(err)] = np.inf
        bad = np.flatnonzero(err > bar)
        flat = np.moveaxis(got, 0, -1).reshape(-1, 2)
        lines = ["%s got %s off by %.3g" % (self.describe(p), flat[p].tolist(), err[p]) for p in bad[:show]]
        return len(bad), "\n".join(lines)
