"""Pixel-by-pixel float64 oracle for the resampling of the semi-Lagrangian extrapolator.  Plain NumPy / SciPy; nothing
here runs on the device.

``resample`` restates pysteps/extrapolation/semilagrangian.py:144-157 and :221-253 at GIVEN coordinates
``grid (+ grid_off) + disp`` formed in float64, so a test can resample the field at the displacement the device itself
returned (an integer plus a float32 fraction: exact in a double).  That takes trajectory drift out of the comparison and
leaves the resampling alone, which can then be held per pixel to a float32 rounding budget:

* order 0: exact equality (the same texel is picked);
* order 1: ``8 u mag`` (u = 2^-24): the blend rounds the weights (1 - f: 1/2 ulp, their products: 1/2 ulp) and the three
  fma partial sums (1/2 ulp of at most ``mag`` each) - below 5 u mag, bar 8 u mag -, with ``mag`` the largest ``|p|``
  over the 2 x 2 tap footprint (``|outval|`` where a tap is the constant);
* orders 2 .. 5: ``4 C_k u mag`` with ``mag`` the largest ``|p|`` of the zeroed field (the prefilter is not local) and
  ``C_k`` MEASURED on the CPU against the reference only: the largest deviation of a float32 restatement of the
  reference's pipeline (``resample_f32``: float32 prefilter, weights and sums) from the float64 SciPy result, in units of
  ``u mag``, over the spline cases of helpers/semilag_pointwise_cases.py.  The factor 4 is for the device ordering the same
  float32 operations differently (segments, transposes, no contraction).  The measured values and the bars live in
  tests/golden/semilag_pointwise_bars.json (``python -m helpers.semilag_pointwise_cases`` from tests/ rewrites it).

Coordinates at which float64 and float32 may legitimately choose differently are skipped (``skip_mask``), and a case may
skip at most ``skip_cap`` pixels.
"""

import json
import os

import numpy as np

EPS32 = 2.0**-24  # unit roundoff of float32
DISP_TOL = 1e-4  # the displacement contract (px)
SAMPLE_ULPS = 8  # order 1, see above
BAR_FACTOR = 4.0  # orders 2 .. 5: bar = BAR_FACTOR * C_k
EDGE_EPS = 1e-6  # px: next to an image edge / a .5 tie
MASK_EPS = 1e-5  # a warped mask next to its 0.5 threshold
BARS_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden",
                         "semilag_pointwise_bars.json")


def _disp_budget(vmax, lip, smax, n_sub):
    """Largest trajectory difference float32 split arithmetic may leave after ``n_sub`` sub-steps.

    Per sub-step the kernel rounds: the bilinear velocity samples (weights 1 - f and their products, three fma's: <= 6
    roundings of at most |V|), the perturbation a V_par + b V_perp (a, b and V_par rounded to float32: <= 4 roundings of
    |V|), the scaling by the step (1), and the two retreats f - w (1/2 ulp of |f - w| <= |V| s + 1 each).  Two velocity
    samples per sub-step: e1 <= 2 * (6 + 4 + 1 + 1) * u * max(|V| s, 1) < 24 u max(|V| s, 1), u = 2^-24.  An error
    already made is carried on and changes the next velocity sample by at most lip * error (lip = the largest
    difference of neighbouring velocity values, the Lipschitz constant of the bilinear interpolant), i.e. it grows by
    (1 + lip s) per sub-step; after N sub-steps: N e1 (1 + lip s)^N.  Capped by the contract.  A calm pixel in a
    moving flow or a sentinel patch is a jump of |V| between neighbours: a trajectory that samples it amplifies what it
    carries by up to (1 + |V| s) per pass (6e-4 px was seen after three calls at 29 px / step), so such trajectories
    (``touched``) are held to (b) and to the sentinel rules only, and lip is taken without those pixels."""
    e1 = 24.0 * EPS32 * max(vmax * smax, 1.0)
    grow = (1.0 + lip * smax) ** n_sub
    return min(n_sub * e1 * grow, DISP_TOL)


# ---- coordinates -------------------------------------------------------------------------------------------------------
def grid_offsets(xy_coords, m, n):
    """``xy_coords - meshgrid`` in float64 (None for the default grid)."""
    if xy_coords is None:
        return None
    xy = np.asarray(xy_coords, dtype=np.float64)
    yy, xx = np.mgrid[0:m, 0:n].astype(np.float64)
    return np.stack([xy[0] - xx, xy[1] - yy])


def coordinates(shape, disp, grid_off=None):
    """(cx, cy) = grid (+ grid_off) + disp in float64 (reference :174-179, :221)."""
    m, n = shape
    yy, xx = np.mgrid[0:m, 0:n].astype(np.float64)
    if grid_off is not None:
        xx, yy = xx + grid_off[0], yy + grid_off[1]
    disp = np.asarray(disp, dtype=np.float64)
    return xx + disp[0], yy + disp[1]


def _lost_value(mode, order, cval):
    """What a NaN coordinate (a lost trajectory) samples: SciPy answers with cval in mode "constant" and with NaN where it
    interpolates across it in mode "nearest" (oracle/semilag.py::_numpy_sample, pinned by the sl_velnan* goldens)."""
    if mode == "constant":
        return cval
    if mode == "nearest" and order >= 1:
        return np.nan
    raise NotImplementedError("non-finite coordinates are restated for modes constant / nearest only")


def _outval(p64, outval):
    if isinstance(outval, str):
        if outval != "min":
            raise ValueError("outval must be a number or 'min'")
        return float(np.nanmin(p64))
    return float(outval)


class _Warps:
    """One resampling: its coordinates and map_coordinates calls, behind ``resample``, ``skip_mask``, ``magnitude``."""

    def __init__(self, precip32, disp, order, mode, outval, grid_off):
        self.p = np.asarray(precip32).astype(np.float64)
        self.order, self.mode = int(order), mode
        self.outval = _outval(self.p, outval)
        self.cx, self.cy = coordinates(self.p.shape, disp, grid_off)
        self.ok = np.isfinite(self.cx) & np.isfinite(self.cy)
        self.rc = [np.where(self.ok, self.cy, 0.0), np.where(self.ok, self.cx, 0.0)]
        self._masks = None

    def warp(self, a, order, cval):
        from scipy.ndimage import map_coordinates

        w = map_coordinates(a, self.rc, order=order, mode=self.mode, cval=cval, prefilter=order > 1)
        if not self.ok.all():
            w = np.where(self.ok, w, _lost_value(self.mode, order, cval))
        return w

    def masks(self):
        """minval and the two order-1 mask warps of the spline orders (reference :146-155, :234-253)."""
        if self._masks is None:
            fin = np.isfinite(self.p)
            minval = np.nanmin(self.p)
            with np.errstate(invalid="ignore"):
                mask_min = (self.p > minval).astype(np.float64)
            self._masks = (minval, self.warp(mask_min, 1, 0.0), self.warp(fin.astype(np.float64), 1, 0.0))
        return self._masks

    def zeroed(self):
        return np.where(np.isfinite(self.p), self.p, 0.0)

    def apply_masks(self, val):
        minval, wmin, wfin = self.masks()
        val = np.array(val, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            val[wmin < 0.5] = minval
            val[wfin < 0.5] = np.nan
        return val

    def resample(self):
        if self.order <= 1:
            return self.warp(self.p, self.order, self.outval)
        return self.apply_masks(self.warp(self.zeroed(), self.order, self.outval))

    def magnitude(self):
        from oracle import semilag as osl

        mode = self.mode
        a = np.abs(self.zeroed())
        m, n = a.shape
        if self.order > 1:
            return np.full((m, n), float(a.max()))
        cmag = abs(self.outval) if np.isfinite(self.outval) else 0.0
        row, col = self.rc
        rr, cc = osl._fold_coordinate(row, m, mode), osl._fold_coordinate(col, n, mode)
        if self.order == 0:
            r0, c0, taps = np.floor(rr + 0.5).astype(np.int64), np.floor(cc + 0.5).astype(np.int64), (0,)
        else:
            r0, c0, taps = np.floor(rr).astype(np.int64), np.floor(cc).astype(np.int64), (0, 1)
        mag = np.zeros((m, n))
        for dr in taps:
            ri, rcv = osl._fold_tap(r0 + dr, m, mode)
            for dc in taps:
                ci, ccv = osl._fold_tap(c0 + dc, n, mode)
                mag = np.maximum(mag, np.where(rcv | ccv, cmag, a[ri, ci]))
        if mode == "constant":
            outside = (row < 0.0) | (row > m - 1.0) | (col < 0.0) | (col > n - 1.0)
            mag = np.where(outside, cmag, mag)
        return np.where(self.ok, mag, cmag)

    def skip(self):
        m, n = self.p.shape
        skip = np.zeros((m, n), bool)
        ties = self.order == 0 or self.order % 2 == 0
        with np.errstate(invalid="ignore"):
            for c, ln in ((self.cx, n), (self.cy, m)):
                for edge in (0.0, ln - 1.0):
                    d = np.abs(c - edge)
                    skip |= (d > 0) & (d <= EDGE_EPS)
                if ties:
                    d = np.abs(c - np.floor(c) - 0.5)
                    skip |= (d > 0) & (d <= EDGE_EPS)
            if self.order > 1:
                _, wmin, wfin = self.masks()
                skip |= (np.abs(wmin - 0.5) <= MASK_EPS) | (np.abs(wfin - 0.5) <= MASK_EPS)
        return skip & self.ok


def resample(precip32, disp, order, mode, outval, grid_off=None):
    """The reference's resampling of ``precip32`` at grid (+ grid_off) + disp, float64 (not rounded to the field's dtype).

    Orders above 1: the non-finite values are zeroed first, the field is sampled with the spline prefilter, and the two
    order-1 mask warps (same mode, cval 0) assign the minimum and then NaN where they are below 0.5.  ``outval="min"`` is
    ``nanmin``.  A NaN coordinate samples ``outval`` (mode "constant")."""
    return _Warps(precip32, disp, order, mode, outval, grid_off).resample()


def skip_mask(precip32, disp, order, mode, outval, grid_off=None):
    """Coordinates where float64 and float32 may legitimately choose differently: within 1e-6 px of an image edge but not
    on it; for even orders and order 0 within 1e-6 of a .5 tie but not on it; for orders above 1 the pixels whose warped
    mask is within 1e-5 of 0.5."""
    return _Warps(precip32, disp, order, mode, outval, grid_off).skip()


def skip_cap(pixels):
    return max(2, 1e-3 * pixels)


# ---- per-pixel magnitude -----------------------------------------------------------------------------------------------
def magnitude(precip32, disp, order, mode, outval, grid_off=None):
    """Orders 0 / 1: the largest ``|p|`` over the (order + 1)^2 tap footprint, ``|outval|`` where a tap (or, in mode
    "constant", the sample) lies outside - a running maximum over the taps, gathered with the oracle's index folding.
    Orders 2 .. 5: the largest absolute value of the zeroed field."""
    return _Warps(precip32, disp, order, mode, outval, grid_off).magnitude()


# ---- bars ---------------------------------------------------------------------------------------------------------------
_BARS = None


def load_bars():
    global _BARS
    if _BARS is None:
        with open(BARS_JSON) as fh:
            _BARS = json.load(fh)
    return _BARS


def bar_ulps(order, bars=None):
    """The bar of an order in units of ``u mag``."""
    if order == 0:
        return 0.0
    if order == 1:
        return float(SAMPLE_ULPS)
    return float((bars or load_bars())["orders"][str(order)]["bar"])


class Reference:
    """want / skip / mag / bar of one resampling."""

    def __init__(self, precip32, disp, order, mode, outval, grid_off=None, bars=None):
        w = _Warps(precip32, disp, order, mode, outval, grid_off)
        self.order, self.mode = w.order, mode
        self.want = w.resample()
        self.skip = w.skip()
        self.mag = w.magnitude()
        self.bar = bar_ulps(w.order, bars) * EPS32 * self.mag
        self.rms = float(np.sqrt(np.mean(w.p[np.isfinite(w.p)] ** 2)))


def pointwise_check(got, ref):
    """Hold ``got`` (one plane) to ``ref`` pixel by pixel.  Returns (largest error in units of its bar, skip count); for
    order 0 the first is 0.0 when every pixel is equal."""
    got = np.asarray(got)
    assert got.shape == ref.want.shape, (got.shape, ref.want.shape)
    nskip = int(ref.skip.sum())
    assert nskip <= skip_cap(ref.skip.size), ("too many coordinates at an edge / a tie / a mask threshold", nskip)
    keep = ~ref.skip
    bad = keep & (np.isnan(got) != np.isnan(ref.want))
    assert not bad.any(), ("NaN mask", int(bad.sum()), [tuple(int(i) for i in k) for k in np.argwhere(bad)[:6]])
    fin = keep & np.isfinite(ref.want)
    if not fin.any():
        return 0.0, nskip
    err = np.abs(got.astype(np.float64) - ref.want)
    over = fin & ~(err <= ref.bar)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(fin, np.where(err == 0.0, 0.0, err / ref.bar), 0.0)
    worst = float(ratio.max())
    if over.any():
        k = np.unravel_index(int(np.argmax(np.where(over, ratio, -1.0))), err.shape)
        raise AssertionError(("pointwise", "order %d" % ref.order, ref.mode, "%d pixels over their bar" % int(over.sum()),
                              "worst at", tuple(int(i) for i in k), "got", float(got[k]), "want", float(ref.want[k]),
                              "err", float(err[k]), "bar", float(ref.bar[k])))
    return worst, nskip


# ---- the float32 restatement that C_k is measured with ---------------------------------------------------------------
def _prefilter_f32(field32, kind, order):
    """oracle/semilag.py::_spline_prefilter (the ni_splines.c recursion) with float32 data, poles and gain."""
    from oracle import semilag as osl

    poles = [float(np.float32(z)) for z in osl._spline_poles(order)]
    gain = 1.0
    for z in osl._spline_poles(order):
        gain *= (1.0 - z) * (1.0 - 1.0 / z)
    c = np.array(field32, dtype=np.float32)
    for axis in (0, 1):
        c = np.moveaxis(c, axis, 0).copy()
        n = c.shape[0]
        if n > 1:
            c *= np.float32(gain)
            for z in poles:
                osl._spline_pole_pass(c, n, z, kind)
            assert c.dtype == np.float32
        c = np.moveaxis(c, 0, axis)
    return c


def resample_f32(precip32, disp, order, mode, outval, grid_off=None):
    """The reference's pipeline for orders 2 .. 5 with the spline arithmetic in float32: float32 prefilter of the zeroed
    (and, for "nearest" / "grid-constant", padded) field, float32 B-spline weights, float32 products and sums over the
    (order + 1)^2 folded taps.  Coordinates, tap indices and the mask decisions are those of the float64 pipeline."""
    from oracle import semilag as osl

    w = _Warps(precip32, disp, order, mode, outval, grid_off)
    assert 2 <= w.order <= 5
    f32 = np.float32
    m, n = w.p.shape
    z32 = w.zeroed().astype(f32)
    npad = osl._PREFILTER_PAD.get(mode, 0)
    if mode == "nearest":
        padded = np.pad(z32, npad, mode="edge")
    elif mode == "grid-constant":
        padded = np.pad(z32, npad, mode="constant", constant_values=f32(w.outval))
    else:
        padded = z32
    with np.errstate(invalid="ignore", over="ignore"):
        coef = _prefilter_f32(padded, osl._PREFILTER_KIND[mode], w.order)
    row, col = w.rc
    rr, cc = osl._fold_coordinate(row, m, mode) + npad, osl._fold_coordinate(col, n, mode) + npad
    big_m, big_n = padded.shape

    def taps(c):
        base = np.floor(c) if w.order & 1 else np.floor(c + 0.5)
        start = base.astype(np.int64) - w.order // 2
        return start, [osl._bspline_basis((c - (start + k)).astype(f32), w.order).astype(f32) for k in range(w.order + 1)]

    iy, wy = taps(rr)
    ix, wx = taps(cc)
    acc = np.zeros((m, n), f32)
    cval32 = f32(w.outval)
    with np.errstate(invalid="ignore"):
        cols = [osl._fold_tap(ix + b, big_n, mode) for b in range(w.order + 1)]
        for a in range(w.order + 1):
            ri, rcv = osl._fold_tap(iy + a, big_m, mode)
            for b, (ci, ccv) in enumerate(cols):
                tap = coef[ri, ci]
                if mode == "grid-constant":
                    tap = np.where(rcv | ccv, cval32, tap)
                acc = acc + (wy[a] * wx[b]) * tap
    assert acc.dtype == f32
    val = acc.astype(np.float64)
    if mode == "constant":
        outside = (row < 0.0) | (row > m - 1.0) | (col < 0.0) | (col > n - 1.0)
        val = np.where(outside, w.outval, val)
    if not w.ok.all():
        val = np.where(w.ok, val, _lost_value(mode, w.order, w.outval))
    return w.apply_masks(val)


def deviation_ulps(precip32, disp, order, mode, outval, grid_off=None):
    """Largest |resample_f32 - resample| in units of ``u mag`` over the pixels a comparison keeps (0.0 if none)."""
    w = _Warps(precip32, disp, order, mode, outval, grid_off)
    want = w.resample()
    got = resample_f32(precip32, disp, order, mode, outval, grid_off)
    keep = ~w.skip()
    assert np.array_equal(np.isnan(got[keep]), np.isnan(want[keep])), "the float32 restatement's NaN mask"
    keep &= np.isfinite(want)
    if not keep.any():
        return 0.0
    mag = float(np.abs(w.zeroed()).max())
    return float(np.max(np.abs(got - want)[keep])) / (EPS32 * mag)
