"""A pointwise yardstick for the RBF evaluation kernel (csrc/rbf.hip, ``rbf_eval<FN>``, entry point
``psh_rbf_eval_dev``): a wide oracle, the unit its error is measured in, a bar per pixel, the fixed list of cases and a
float64 NumPy model of the kernel with switchable seeded defects (tests/test_rbf_cpu.py shows that the check rejects
each of them).

The quantity
------------
``x0, dx, y0, dy``, the node coordinates ``(x_j, y_j)`` and the weights ``w_j`` are float64.  For pixel ``(iy, ix)``,
with ``x = x0 + dx ix``, ``y = y0 + dy iy`` and ``r2_j = (x - x_j)^2 + (y - y_j)^2`` the kernel computes
``S = sum_j w_j phi(r2_j)`` for two weight columns at once (the second one stored a plane further).

The oracle is that sum in ``numpy.longdouble`` (64-bit significand, asserted the way helpers/moments.py does): the
inputs convert exactly, ``1 / eps^2`` is formed in longdouble from the float64 ``epsilon``.  Where longdouble is no
wider than float64 the oracle is mpmath at 50 digits on a fixed sample of at most 2000 pixels per case (always the four
corners, the last row and the last column); the pixels outside the sample are then not judged.

The bar (derived, not measured)
-------------------------------
The weights of an RBF system alternate in sign, ``|S|`` can be 1e16 times smaller than its terms: the error is
normalised by the sum of magnitudes, ``B = sum_j |w_j| A(r2_j)``, with

* ``A = |phi|`` for multiquadric, inverse, linear, cubic and quintic,
* ``A = phi (1 + r2 / eps^2)`` for gaussian: a relative error d in the exponent t costs t d in the value,
* ``A = 0.5 r2 (|ln r2| + 1)`` for thin_plate (0 at r2 = 0): phi crosses zero at r = 1, its absolute error does not.

With u = 2^-53 the bar is ``|got - S| <= (N + 16) u B`` at every pixel of both planes:

* ``N u`` for the chain of N fmas (each adds one rounding of a partial sum that is at most B),
* ``16 u`` for phi itself: r2 costs 4 u (one rounding in each difference, one in ddx^2, one in the fma),
  ``1 / (eps eps)`` costs 2 u, the worst conditioning is quintic's ``r2 r2 sqrt(r2)`` (2.5 x the error of r2 plus
  three roundings: 13 u), and OCML's double sqrt, exp and log are taken at <= 2 ulp from their documentation.

That model (every operation returns its result times 1 + d, |d| <= u) holds where nothing underflows.  A Gaussian
term below the smallest normal number may be flushed to zero or lose bits, an absolute error of at most 2^-1022 per
term, so the bar carries ``sum_j |w_j| 2^-1022`` as well - 1e-308 per unit of weight, nothing on any case but the
Gaussian with a tiny epsilon, where the float64 terms underflow while longdouble's (15-bit exponent) do not.

The bar holds as stated on grids where ``x0 + dx ix`` is exact in float64 (integers, dyadic fractions, whole metres):
there the compiler's choice between fma and mul + add for the pixel coordinate cannot matter.  On an inexact grid the
oracle is evaluated at the real ``x0 + dx i`` and the bar gains the coordinate term
``sum_j |w_j| |dphi/dr|(r_j) (delta_x + delta_y)`` with ``delta_x = u (|x0| + 2 |dx| ix)`` (one rounding of the product
and one of the sum, the latter bounded by the larger of the two operands' sum) and likewise delta_y; the derivatives:
mq ``(r/e^2) / sqrt(1 + (r/e)^2)``, inverse ``(r/e^2) / (1 + (r/e)^2)^1.5``, gaussian ``2 r / e^2 exp(-(r/e)^2)``,
linear ``1``, cubic ``3 r^2``, quintic ``5 r^4``, thin_plate ``r |2 ln r + 1|``.

If the device exceeds the bar, that is a finding about the kernel; the constant moves only if this derivation is shown
wrong on paper.  tests/test_rbf_cpu.py asserts that honest float64 evaluations (three summation orders, SciPy's own)
stay below a quarter of it on every case: a condition on the inputs, checked and not assumed.
"""

import functools
import warnings
from dataclasses import dataclass, field

import numpy as np

from helpers.moments import wide_longdouble

FUNCTIONS = ("multiquadric", "inverse", "gaussian", "linear", "cubic", "quintic", "thin_plate")
CODE = {name: i for i, name in enumerate(FUNCTIONS)}
EPSILON_BEARING = FUNCTIONS[:3]
U = 2.0 ** -53
TINY = 2.0 ** -1022  # smallest normal float64
PHI_COST = 16
CHUNK = 256          # nodes staged in LDS at a time
TILE_X, TILE_Y, ROWS_PER_THREAD = 64, 16, 4
MP_SAMPLE = 2000
ORDERS = ("forward", "reversed", "pairwise")
DEFECTS = ("drop_chunk_tail", "row_stride", "second_var_reads_first", "phi_float32", "thin_plate_nan_at_zero",
           "last_column_stale", "gaussian_eps_not_squared")

LD = np.longdouble


# ---- basis functions in longdouble ---------------------------------------------------------------------------------

def _inv_eps2(function, epsilon):
    if function not in EPSILON_BEARING:
        return LD(0.0)
    e = LD(float(epsilon))
    return LD(1.0) / (e * e)


def _safe_log(r2):
    return np.log(np.where(r2 > 0, r2, LD(1.0)))


def phi_ld(r2, function, inv_eps2):
    """phi(r2) of scipy.interpolate.Rbf's ``_h_<function>`` on a longdouble array of squared distances."""
    r2 = np.asarray(r2, dtype=LD)
    if function == "multiquadric":
        return np.sqrt(r2 * inv_eps2 + LD(1.0))
    if function == "inverse":
        return LD(1.0) / np.sqrt(r2 * inv_eps2 + LD(1.0))
    if function == "gaussian":
        return np.exp(-(r2 * inv_eps2))
    if function == "linear":
        return np.sqrt(r2)
    if function == "cubic":
        return r2 * np.sqrt(r2)
    if function == "quintic":
        return r2 * r2 * np.sqrt(r2)
    if function == "thin_plate":
        return LD(0.5) * r2 * _safe_log(r2)  # 0 at r2 = 0
    raise ValueError(function)


def unit_ld(r2, function, inv_eps2):
    """A(r2): the magnitude an error of phi is relative to (module docstring)."""
    if function == "gaussian":
        return phi_ld(r2, function, inv_eps2) * (LD(1.0) + r2 * inv_eps2)
    if function == "thin_plate":
        return LD(0.5) * r2 * (np.abs(_safe_log(r2)) + LD(1.0))
    return np.abs(phi_ld(r2, function, inv_eps2))


def dphi_dr_ld(r2, function, inv_eps2):
    """|dphi/dr| at r = sqrt(r2)."""
    r = np.sqrt(r2)
    t = r2 * inv_eps2
    if function == "multiquadric":
        return r * inv_eps2 / np.sqrt(LD(1.0) + t)
    if function == "inverse":
        return r * inv_eps2 / ((LD(1.0) + t) * np.sqrt(LD(1.0) + t))
    if function == "gaussian":
        return LD(2.0) * r * inv_eps2 * np.exp(-t)
    if function == "linear":
        return np.ones_like(r)
    if function == "cubic":
        return LD(3.0) * r2
    if function == "quintic":
        return LD(5.0) * r2 * r2
    if function == "thin_plate":
        return r * np.abs(_safe_log(r2) + LD(1.0))  # r |2 ln r + 1|
    raise ValueError(function)


# ---- the oracle ----------------------------------------------------------------------------------------------------

def _pixels(m, n, pixels):
    if pixels is None:
        iy, ix = np.divmod(np.arange(m * n), n)
    else:
        iy, ix = (np.asarray(p, dtype=np.int64).reshape(-1) for p in pixels)
    return iy, ix


def _reduce(xy, w, m, n, x0, dx, y0, dy, function, epsilon, pixels, what, block=1024):
    """sum_j over the nodes of (w_j phi, |w_j| A) or of |w_j| |dphi/dr|, per pixel and weight column, in longdouble."""
    assert wide_longdouble()
    xy, w = np.asarray(xy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    iy, ix = _pixels(m, n, pixels)
    inv = _inv_eps2(function, epsilon)
    xj, yj = xy[:, 0].astype(LD), xy[:, 1].astype(LD)
    wl, wa = w.astype(LD), np.abs(w).astype(LD)
    out = [np.empty((2, iy.size), dtype=LD) for _ in range(2 if what == "sum" else 1)]
    for p0 in range(0, iy.size, block):
        x = LD(float(x0)) + LD(float(dx)) * ix[p0:p0 + block].astype(LD)
        y = LD(float(y0)) + LD(float(dy)) * iy[p0:p0 + block].astype(LD)
        ddx, ddy = x[:, None] - xj[None, :], y[:, None] - yj[None, :]
        r2 = np.ascontiguousarray(ddx * ddx + ddy * ddy)
        if what == "sum":
            phi, a = phi_ld(r2, function, inv), unit_ld(r2, function, inv)
            for k in range(2):
                out[0][k, p0:p0 + block] = np.sum(phi * wl[None, :, k], axis=1)
                out[1][k, p0:p0 + block] = np.sum(a * wa[None, :, k], axis=1)
        else:
            d = dphi_dr_ld(r2, function, inv)
            for k in range(2):
                out[0][k, p0:p0 + block] = np.sum(d * wa[None, :, k], axis=1)
    return out


def _shape(a, m, n, pixels):
    return a.reshape(2, m, n) if pixels is None else a


def mp_sample(m, n):
    """The fixed sample of the mpmath route: corners, last row, last column and seeded random pixels, <= MP_SAMPLE."""
    if m * n <= MP_SAMPLE:
        return np.divmod(np.arange(m * n), n)
    flat = set([0, n - 1, (m - 1) * n, m * n - 1]) | set(range((m - 1) * n, m * n)) | set(range(n - 1, m * n, n))
    assert len(flat) <= MP_SAMPLE
    rest = np.random.default_rng([m, n]).permutation(m * n)
    for p in rest:
        if len(flat) >= MP_SAMPLE:
            break
        flat.add(int(p))
    return np.divmod(np.array(sorted(flat)), n)


def _ld_to_mp(mp, v):
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))


def oracle_mp(xy, w, m, n, x0, dx, y0, dy, function, epsilon, pixels):
    """(S, B) at the listed pixels with mpmath at 50 digits, as lists of mpf per weight column: ``S[k][p]``."""
    import mpmath

    mp = mpmath.mp.clone()
    mp.dps = 50
    f = mp.mpf
    xy, w = np.asarray(xy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    iy, ix = _pixels(m, n, pixels)
    inv = 1 / (f(float(epsilon)) ** 2) if function in EPSILON_BEARING else f(0)
    nodes = [(f(float(a)), f(float(b))) for a, b in xy]
    ws = [(f(float(a)), f(float(b))) for a, b in w]

    def phi_a(r2):
        if function == "multiquadric":
            v = mp.sqrt(r2 * inv + 1)
            return v, v
        if function == "inverse":
            v = 1 / mp.sqrt(r2 * inv + 1)
            return v, v
        if function == "gaussian":
            v = mp.exp(-(r2 * inv))
            return v, v * (1 + r2 * inv)
        if function == "linear":
            v = mp.sqrt(r2)
            return v, v
        if function == "cubic":
            v = r2 * mp.sqrt(r2)
            return v, v
        if function == "quintic":
            v = r2 * r2 * mp.sqrt(r2)
            return v, v
        if r2 == 0:
            return f(0), f(0)
        return r2 * mp.log(r2) / 2, r2 * (abs(mp.log(r2)) + 1) / 2

    S, B = ([], []), ([], [])
    for py_, px_ in zip(iy, ix):
        x, y = f(float(x0)) + f(float(dx)) * int(px_), f(float(y0)) + f(float(dy)) * int(py_)
        s, b = [f(0), f(0)], [f(0), f(0)]
        for (a, c), wj in zip(nodes, ws):
            p, q = phi_a((x - a) ** 2 + (y - c) ** 2)
            for k in range(2):
                s[k] += wj[k] * p
                b[k] += abs(wj[k]) * q
        for k in range(2):
            S[k].append(s[k])
            B[k].append(b[k])
    return S, B


def oracle(xy, w, N, m, n, x0, dx, y0, dy, function, epsilon, pixels=None):
    """(S, B): the interpolant and its unit, ``(2, m, n)`` each (``(2, P)`` for ``pixels=(iy, ix)``), in longdouble.

    Without a 64-bit significand: mpmath on :func:`mp_sample` (or the listed pixels), NaN at the pixels left out."""
    assert np.shape(xy) == (N, 2) and np.shape(w) == (N, 2), (np.shape(xy), np.shape(w), N)
    if wide_longdouble():
        S, B = _reduce(xy, w, m, n, x0, dx, y0, dy, function, epsilon, pixels, "sum")
        return _shape(S, m, n, pixels), _shape(B, m, n, pixels)
    sample = mp_sample(m, n) if pixels is None else _pixels(m, n, pixels)
    Sm, Bm = oracle_mp(xy, w, m, n, x0, dx, y0, dy, function, epsilon, sample)
    if pixels is not None:
        return (np.array([[LD(float(v)) for v in col] for col in Sm]),
                np.array([[LD(float(v)) for v in col] for col in Bm]))
    S, B = np.full((2, m, n), np.nan, dtype=LD), np.full((2, m, n), np.nan, dtype=LD)
    for k in range(2):
        S[k][sample] = [float(v) for v in Sm[k]]
        B[k][sample] = [float(v) for v in Bm[k]]
    return S, B


def bar(xy, w, N, m, n, x0, dx, y0, dy, function, epsilon, B, coordinate=False, pixels=None):
    """The bar per pixel (module docstring): ``(N + 16) u B`` plus the underflow term, plus, with ``coordinate``, what a
    rounding of the pixel coordinates costs."""
    w = np.asarray(w, dtype=np.float64)
    out = LD(N + PHI_COST) * LD(U) * B
    under = np.abs(w).astype(LD).sum(axis=0) * LD(TINY)
    out = out + under.reshape((2,) + (1,) * (out.ndim - 1))
    if coordinate:
        iy, ix = _pixels(m, n, pixels)
        if wide_longdouble():
            (D,) = _reduce(xy, w, m, n, x0, dx, y0, dy, function, epsilon, pixels, "slope")
        else:  # the slope enters a bound only: float64 is enough for it
            D = _slope_float64(xy, w, x0, dx, y0, dy, function, epsilon, iy, ix)
        delta = LD(U) * ((abs(float(x0)) + 2.0 * abs(float(dx)) * ix) + (abs(float(y0)) + 2.0 * abs(float(dy)) * iy))
        out = out + _shape(D * delta[None, :], m, n, pixels)
    return out


def _slope_float64(xy, w, x0, dx, y0, dy, function, epsilon, iy, ix):
    inv = float(_inv_eps2(function, epsilon))
    r2 = (x0 + dx * ix[:, None] - xy[None, :, 0]) ** 2 + (y0 + dy * iy[:, None] - xy[None, :, 1]) ** 2
    d = np.asarray(dphi_dr_ld(r2.astype(LD), function, LD(inv)))
    return np.stack([np.sum(d * np.abs(w[None, :, k]), axis=1) for k in range(2)])


def check(got, S, Bar):
    """(worst ``|got - S| / Bar``, its index): passes when the ratio is <= 1.  A non-finite ``got`` and any error where
    the bar is zero count as infinite.  Pixels the mpmath route left out (NaN in S) are not judged."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == S.shape == Bar.shape, (got.shape, S.shape, Bar.shape)
    err = np.abs(got.astype(LD) - S)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(Bar > 0, err / np.where(Bar > 0, Bar, LD(1.0)), np.where(err == 0, LD(0.0), LD(np.inf)))
    ratio = np.where(np.isfinite(got), ratio, LD(np.inf))
    if not wide_longdouble():
        ratio = np.where(np.isnan(S), LD(0.0), ratio)
    else:
        assert np.isfinite(S).all()
    k = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[k]), tuple(int(i) for i in np.unravel_index(k, ratio.shape))


# ---- cases ---------------------------------------------------------------------------------------------------------

@dataclass(eq=False)
class Case:
    name: str
    function: str
    xy: np.ndarray        # (N, 2) float64
    w: np.ndarray         # (N, 2) float64
    m: int
    n: int
    x0: float = 0.0
    dx: float = 1.0
    y0: float = 0.0
    dy: float = 1.0
    epsilon: float = 1.0
    values: np.ndarray = None   # the samples SciPy solved for (None: synthetic weights)
    rbfi: object = None         # the scipy.interpolate.Rbf whose nodes the weights are, untouched
    coordinate: bool = False    # inexact grid: the bar carries the coordinate term
    on_nodes: bool = False      # every node is a pixel
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def N(self):
        return self.xy.shape[0]

    def geometry(self):
        return self.m, self.n, self.x0, self.dx, self.y0, self.dy

    def yardstick(self):
        """(S, Bar, B) of the case, computed once."""
        if "y" not in self._cache:
            S, B = oracle(self.xy, self.w, self.N, *self.geometry(), self.function, self.epsilon)
            Bar = bar(self.xy, self.w, self.N, *self.geometry(), self.function, self.epsilon, B, coordinate=self.coordinate)
            for a in (S, B, Bar):
                a.setflags(write=False)
            self._cache["y"] = (S, Bar, B)
        return self._cache["y"]

    def node_pixels(self):
        """(iy, ix) of the nodes of an on-node case."""
        assert self.on_nodes
        ix = np.rint((self.xy[:, 0] - self.x0) / self.dx).astype(int)
        iy = np.rint((self.xy[:, 1] - self.y0) / self.dy).astype(int)
        assert np.array_equal(self.x0 + self.dx * ix, self.xy[:, 0]) and np.array_equal(self.y0 + self.dy * iy, self.xy[:, 1])
        return iy, ix


def _seed(*parts):
    return [sum(ord(c) * (i + 1) for i, c in enumerate(str(p))) for p in parts]


def _jittered(N, span_x, span_y, rng):
    """One node per cell of a coarse lattice over [0, span_x] x [0, span_y], jittered off every grid line."""
    side = int(np.ceil(np.sqrt(N)))
    cells = rng.permutation(side * side)[:N]
    cy, cx = np.divmod(cells, side)
    return np.column_stack([(cx + rng.random(N)) * span_x / side, (cy + rng.random(N)) * span_y / side])


def _values(N, rng):
    return rng.normal(0.0, 2.0, (N, 2)) + np.array([2.0, -1.0])


def default_epsilon(xy):
    """scipy.interpolate.Rbf's default: the average distance between nodes, from the bounding box."""
    edges = xy.max(axis=0) - xy.min(axis=0)
    edges = edges[np.nonzero(edges)]
    return float(np.power(np.prod(edges) / xy.shape[0], 1.0 / edges.size))


def solve(xy, values, function, epsilon=None, smooth=0.0):
    """SciPy's own solve: the Rbf object (``.nodes`` (N, 2) weights, ``.epsilon``)."""
    from scipy.interpolate import Rbf

    kw = {} if epsilon is None else {"epsilon": epsilon}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # an ill-conditioned system is what some cases are about
        return Rbf(xy[:, 0], xy[:, 1], values, function=function, smooth=smooth, mode="N-D", **kw)


def _solved(name, function, xy, values, m, n, epsilon=None, **kw):
    rbfi = solve(xy, values, function, epsilon)
    w = np.ascontiguousarray(np.asarray(rbfi.nodes, dtype=np.float64).reshape(xy.shape[0], 2))
    assert np.isfinite(w).all(), (name, function)
    return Case(name, function, np.ascontiguousarray(xy), w, m, n, epsilon=float(rbfi.epsilon), values=values, rbfi=rbfi, **kw)


def _alternating(N, rng):
    w = np.abs(rng.normal(size=(N, 2))) * 10.0 ** rng.uniform(-6.0, 6.0, (N, 2))
    return w * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None]


def _on_node_inputs(m, n, rng, N=300):
    xy = np.round(_jittered(N, n - 1, m - 1, rng))
    _, keep = np.unique(xy, axis=0, return_index=True)
    keep = np.sort(keep)
    return xy[keep], _values(N, rng)[keep]


@functools.lru_cache(maxsize=None)
def cases(function):
    """The fixed case list of a basis function: deterministic, every case seeded and named."""
    assert function in FUNCTIONS
    out = []

    def rng_of(name):
        return np.random.default_rng(_seed(name, function))

    for m, n in ((17, 65), (15, 63), (16, 64)):  # one past the tile, one short of it, the tile itself
        name = "tile-edges-%dx%d" % (m, n)
        rng = rng_of(name)
        xy, values = _jittered(60, n - 1, m - 1, rng), _values(60, rng)
        out.append(_solved(name, function, xy, values, m, n))
        if function in EPSILON_BEARING:
            for eps in (1e-3, 1e6):
                out.append(_solved("%s-eps%g" % (name, eps), function, xy, values, m, n, epsilon=eps))
    for m, n in ((1, 130), (33, 1), (1, 1)):
        name = "thin-%dx%d" % (m, n)
        rng = rng_of(name)
        xy = _jittered(3, max(n - 1, 4), max(m - 1, 4), rng)  # distinct nodes, beside the grid where it has no extent
        out.append(_solved(name, function, xy, _values(3, rng), m, n))
    for N in (255, 256, 257, 513):
        name = "chunk-N%d" % N
        rng = rng_of(name)
        xy = _jittered(N, 64, 32, rng)
        if N <= 257:
            out.append(_solved(name, function, xy, _values(N, rng), 33, 65))
        else:
            out.append(Case(name, function, xy, _alternating(N, rng), 33, 65, epsilon=default_epsilon(xy)))
    rng = rng_of("on-nodes")
    xy, values = _on_node_inputs(50, 70, rng)
    out.append(_solved("on-nodes", function, xy, values, 50, 70, on_nodes=True))
    if function == "gaussian":  # every term but a node's own (and its direct neighbours') underflows in float64
        out.append(_solved("on-nodes-eps0.05", function, xy, values, 50, 70, epsilon=0.05, on_nodes=True))
    rng = rng_of("outside")
    inside = _jittered(20, 69, 19, rng)
    far = []
    while len(far) < 20:  # up to 3 grid widths away, not within the grid rectangle
        p = rng.uniform([-3 * 69.0, -3 * 19.0], [4 * 69.0, 4 * 19.0])
        if not (0.0 <= p[0] <= 69.0 and 0.0 <= p[1] <= 19.0):
            far.append(p)
    out.append(_solved("outside", function, np.vstack([inside, np.array(far)]), _values(40, rng), 20, 70))
    rng = rng_of("metres")
    idx = _jittered(257, 64, 32, rng)
    geo = dict(x0=255000.0, dx=1000.0, y0=500000.0, dy=-1000.0)  # projected metres, descending y
    xy = np.column_stack([geo["x0"] + geo["dx"] * idx[:, 0], geo["y0"] + geo["dy"] * idx[:, 1]])
    out.append(_solved("metres", function, xy, _values(257, rng), 33, 65, **geo))
    rng = rng_of("dyadic")
    idx = _jittered(60, 69, 19, rng)
    geo = dict(x0=-3.25, dx=0.75, y0=10.5, dy=0.5)
    xy = np.column_stack([geo["x0"] + geo["dx"] * idx[:, 0], geo["y0"] + geo["dy"] * idx[:, 1]])
    out.append(_solved("dyadic", function, xy, _values(60, rng), 20, 70, **geo))
    rng = rng_of("inexact")
    xg, yg = np.linspace(-3.0, 250.0, 200), np.linspace(10.0, 80.0, 64)
    geo = dict(x0=float(xg[0]), dx=float((xg[-1] - xg[0]) / 199), y0=float(yg[0]), dy=float((yg[-1] - yg[0]) / 63))
    idx = _jittered(50, 199, 63, rng)
    xy = np.column_stack([geo["x0"] + geo["dx"] * idx[:, 0], geo["y0"] + geo["dy"] * idx[:, 1]])
    out.append(_solved("inexact", function, xy, _values(50, rng), 64, 200, coordinate=True, **geo))
    rng = rng_of("zero-second")
    c = _solved("zero-second", function, _jittered(60, 64, 16, rng), _values(60, rng), 17, 65)
    w = c.w.copy()
    w[:, 1] = 0.0
    out.append(Case("zero-second", function, c.xy, w, 17, 65, epsilon=c.epsilon))
    rng = rng_of("dynamic-range")
    xy, w = _jittered(64, 64, 16, rng), rng.normal(size=(64, 2))
    w[17, 0], w[40, 1] = 1e12, -1e12  # one weight twelve decades above the rest, per column
    out.append(Case("dynamic-range", function, xy, w, 17, 65, epsilon=default_epsilon(xy)))
    for c in out:
        for a in (c.xy, c.w):
            a.setflags(write=False)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(function, name):
    return next(c for c in cases(function) if c.name == name)


# ---- a float64 model of the kernel, with seeded defects ----------------------------------------------------------------

def _phi64(r2, function, inv, guard=True):
    with np.errstate(divide="ignore", invalid="ignore"):
        if function == "multiquadric":
            return np.sqrt(r2 * inv + 1.0)
        if function == "inverse":
            return 1.0 / np.sqrt(r2 * inv + 1.0)
        if function == "gaussian":
            return np.exp(-(r2 * inv))
        if function == "linear":
            return np.sqrt(r2)
        if function == "cubic":
            return r2 * np.sqrt(r2)
        if function == "quintic":
            return r2 * r2 * np.sqrt(r2)
        v = 0.5 * r2 * np.log(r2)
        return np.where(r2 > 0.0, v, 0.0) if guard else v


def _pairwise(t):
    while t.shape[0] > 1:
        half = t.shape[0] // 2
        head = t[:half] + t[half:2 * half]
        t = head if t.shape[0] % 2 == 0 else np.concatenate([head, t[2 * half:]])
    return t[0]


def emulate(case, order="forward", defect=None):
    """The kernel in float64 NumPy (mul + add where the kernel may contract to fma): ``(2, m, n)``.

    ``order``: the order the node terms are summed in.  ``defect``: one of DEFECTS, the seeded mistakes the check has
    to reject (module docstring of tests/test_rbf_cpu.py); a defect that does not apply to the case changes nothing."""
    assert order in ORDERS and (defect is None or defect in DEFECTS)
    c = case
    m, n, N = c.m, c.n, c.N
    rows = np.arange(m)
    if defect == "row_stride":  # a thread's q-th pixel taken from row iy0 + q, stored at iy0 + 4 q
        in_tile = rows % TILE_Y
        rows = rows - in_tile + in_tile % ROWS_PER_THREAD + in_tile // ROWS_PER_THREAD
    nodes = N - 1 if defect == "drop_chunk_tail" and N % CHUNK == 1 else N
    if function_has_eps(c.function):
        inv = 1.0 / c.epsilon if defect == "gaussian_eps_not_squared" and c.function == "gaussian" else 1.0 / (c.epsilon * c.epsilon)
    else:
        inv = 0.0
    px, py = c.x0 + c.dx * np.arange(n, dtype=np.float64), c.y0 + c.dy * rows.astype(np.float64)
    ddx, ddy = px[None, None, :] - c.xy[:nodes, 0, None, None], py[None, :, None] - c.xy[:nodes, 1, None, None]
    r2 = ddy * ddy + ddx * ddx
    phi = _phi64(r2, c.function, inv, guard=defect != "thin_plate_nan_at_zero")
    if defect == "phi_float32":
        phi = phi.astype(np.float32).astype(np.float64)
    out = np.empty((2, m, n))
    for k in range(2):
        t = c.w[:nodes, k, None, None] * phi
        if order == "pairwise":
            out[k] = _pairwise(t)
        else:
            acc = np.zeros((m, n))
            for j in (range(nodes) if order == "forward" else range(nodes - 1, -1, -1)):
                acc = acc + t[j]
            out[k] = acc
    if defect == "second_var_reads_first":
        out[1] = out[0]
    if defect == "last_column_stale" and n % TILE_X == 1:
        out[:, :, n - 1] = 0.0  # what the buffer held before
    return out


def function_has_eps(function):
    return function in EPSILON_BEARING


def scipy_eval(case):
    """SciPy's own ``Rbf.__call__`` on the case's grid: ``(2, m, n)``."""
    c = case
    xg, yg = np.meshgrid(c.x0 + c.dx * np.arange(c.n), c.y0 + c.dy * np.arange(c.m))
    return np.moveaxis(np.asarray(c.rbfi(xg, yg)), -1, 0)
