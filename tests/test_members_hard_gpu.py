"""Member-batched advection (csrc/semilag_members.hip) against the float64 oracle on hard cases.

Every case runs through the four routes into the member kernels - packed planes + compact records with two members
per thread (``members_variant`` 2, the default: semilag_members_pair), one member per thread (``members_variant`` 1),
one plane per component (``packed=False``) and the float64-displacement entry point ``psh_semilag_members_dev`` - and
each route is held against per-member calls of ``oracle/semilag.py`` (SciPy backend) on the member's perturbed motion
field ``V + generate_bps(...)`` formed in float64, with the same steps, ``n_iter``, ``outval`` and displacement chain.

Two things are checked apart so that both bars can be tight:

(a) trajectories: the device displacement against the oracle's, in pixels, where the oracle's is finite and sane;
(b) resampling: the last plane of a call against a float64 ``map_coordinates`` of the member at grid + the DEVICE's own
    displacement (exact: int32 + float32 fraction in a double), which takes trajectory drift out of the comparison.

Every plane is also compared with the oracle's (NaN masks, relative L2).  The bars come from the float32 error budget
(``_disp_budget``, ``_SAMPLE_ULPS``, ``_field_budget``) under the 1e-4 contract of tests/test_semilag_gpu.py; what was
seen is appended to members_hard_seen.jsonl in the directory named by PYSTEPS_HIP_SEEN_DIR, when that is set.
"""

import json
import os

import numpy as np
import pytest

from conftest import nan_mismatch, rel_l2
from helpers.bps import generate_bps
from helpers.semilag_pointwise import EPS32, _disp_budget

pytestmark = pytest.mark.gpu

REL_L2_TOL = 1e-4  # the contract (BASELINE.json north_star)
ROUTES = ("pair", "single", "unpacked", "f64")
NAN_EDGE = 2  # NaN-mask pixels a plane may differ by (test_ensemble_gpu.py: an edge crossed at an exact integer)
_SAMPLE_ULPS = 8  # (b): bilinear blend in float32, see _check_call


def _seen(rec):
    out_dir = os.environ.get("PYSTEPS_HIP_SEEN_DIR")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        rec = dict(rec, test=os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0])
        with open(os.path.join(out_dir, "members_hard_seen.jsonl"), "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _perts(B, seed=5):
    """Asymmetric eps_par / eps_perp of both signs, so that a sign or V_perp orientation error shows."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(B):
        ep = (0.9 + 0.3 * rng.random()) * (-1) ** j
        eq = (-0.35 - 0.4 * rng.random()) * (-1) ** (j // 2)
        out.append(dict(eps_par=ep, eps_perp=eq, p_par=(10.88, 0.23, -7.68), p_perp=(5.76, 0.31, -2.72), vsf=12.0))
    return out


# ---- the device side ---------------------------------------------------------------------------------------------------
class _Device:
    """One route into the member kernels; step() returns the planes (B, T, m, n) (None for a displacement-only call)
    and the displacement (B, 2, m, n) float64 on the host."""

    def __init__(self, route, V, B, perts, n_iter, order, outval):
        from pysteps_amd import _lib
        from pysteps_amd.device import DeviceArray
        from pysteps_amd.extrapolation.ensemble import EnsembleAdvector

        self.route, self.B, self.perts = route, B, perts
        self.m, self.n = V.shape[1:]
        self.n_iter, self.order, self.outval = n_iter, order, outval
        self.lib = _lib.lib()
        if route == "f64":
            self.vel = DeviceArray.from_host(V, np.float32)
            self.vhat = None
            if perts is not None:
                self.vhat = DeviceArray((2, self.m, self.n), np.float32)
                _lib.check(self.lib.psh_velocity_unit_dev(self.vel.ptr, self.m, self.n, self.vhat.ptr), "velocity_unit")
            self.disp = DeviceArray((B, 2, self.m, self.n), np.float64).fill_bytes(0)
            self.started = False
        else:
            self.adv = EnsembleAdvector(V, B, perts, n_iter=n_iter, interp_order=order, outval=outval,
                                        packed=route != "unpacked")
            assert (self.adv.packed is None) == (route == "unpacked")

    def step(self, members, incs, t_total):
        from pysteps_amd import _lib
        from pysteps_amd.device import DeviceArray
        from pysteps_amd.extrapolation.ensemble import bps_scalars

        B, m, n, T = self.B, self.m, self.n, len(incs)
        if self.route != "f64":
            if self.route == "single":
                _lib.check(self.lib.psh_set_option(b"members_variant", 1))
            try:
                out = self.adv.step(members, list(incs), t_total)
            finally:
                _lib.check(self.lib.psh_set_option(b"members_variant", 2))
            disp = np.array(self.adv.displacement.to_host())
            return (None if out is None else np.array(out).reshape(B, T, m, n)), disp
        steps = np.asarray(incs, dtype=np.float64)
        par = perp = None
        if self.perts is not None:
            par, perp = bps_scalars(self.perts, t_total)
        pm = None if members is None else DeviceArray.from_host(members, np.float32)
        out = None if members is None else DeviceArray((B, T, m, n), np.float32)
        rc = self.lib.psh_semilag_members_dev(
            None if pm is None else pm.ptr, self.vel.ptr, None if self.vhat is None else self.vhat.ptr,
            None if par is None else par.ctypes.data, None if perp is None else perp.ctypes.data, B, m, n,
            steps.ctypes.data, T, self.n_iter, self.order, self.outval, self.disp.ptr, int(self.started),
            None if out is None else out.ptr)
        _lib.check(rc, "psh_semilag_members_dev")
        self.started = True
        return (None if out is None else np.array(out.to_host())), np.array(self.disp.to_host())


# ---- the oracle side ---------------------------------------------------------------------------------------------------
class _Oracle:
    """Per-member calls of oracle/semilag.py::extrapolate (SciPy, float64) with the member's own displacement chain."""

    def __init__(self, V, B, perts, n_iter, order, outval, special=None):
        self.V64 = V.astype(np.float64)
        self.B, self.perts, self.n_iter, self.order, self.outval = B, perts, n_iter, order, outval
        self.special = special
        self.D = [None] * B
        self.Dp = [None] * B  # the same chains with NaN at the special pixels: NaN marks a trajectory that sampled them
        self.lip = 0.0  # largest neighbour difference of any member's velocity away from the special pixels (px/px/step)
        self.vmax = 0.0

    def velocity(self, j, t_total):
        if self.perts is None:
            return self.V64
        return self.V64 + generate_bps(self.V64, self.perts[j], t_total)

    def step(self, members, incs, t_total):
        """-> planes (B, T, m, n) or None, displacement (B, 2, m, n), touched (B, m, n): the trajectories that sampled
        a special pixel (a calm pixel in a moving flow, a sentinel patch) with any weight."""
        from oracle import semilag as osl

        ts = [float(t) for t in np.cumsum(incs)]
        outs, disps, touched = [], [], []
        kw = dict(allow_nonfinite_values=True, n_iter=self.n_iter, return_displacement=True, interp_order=self.order,
                  backend="scipy")
        for j in range(self.B):
            Vj = self.velocity(j, t_total)
            probe = Vj.copy()
            if self.special is not None:
                probe[:, self.special] = np.nan
            with np.errstate(all="ignore"):
                self.vmax = max(self.vmax, float(np.nanmax(np.abs(probe))))
                for ax in (1, 2):
                    if Vj.shape[ax] > 1:
                        d = np.abs(np.diff(probe, axis=ax))
                        if np.isfinite(d).any():
                            self.lip = max(self.lip, float(np.nanmax(d)))
                out, self.D[j] = osl.extrapolate(None if members is None else members[j], Vj, ts, outval=self.outval,
                                                 displacement_prev=self.D[j], **kw)
                if self.special is not None:
                    _, self.Dp[j] = osl.extrapolate(None, probe, ts, displacement_prev=self.Dp[j], **kw)
            outs.append(out)
            disps.append(self.D[j])
            touched.append(np.zeros(Vj.shape[1:], bool) if self.special is None else np.isnan(self.Dp[j]).any(axis=0))
        return (None if members is None else np.stack(outs)), np.stack(disps), np.stack(touched)


# ---- error budget ------------------------------------------------------------------------------------------------------
def _field_budget(member, disp_bar):
    """rel-L2 a plane may differ from the oracle's: a position error <= d moves a bilinear sample by at most
    d (|dp/dx| + |dp/dy|) of its cell, so the L2 norm of the difference is at most d ||grad||_2 (neighbour differences
    of the member, both axes), plus the blend's own rounding (_SAMPLE_ULPS u of the magnitude), relative to the RMS of
    the finite field.  Capped by the contract."""
    fin = member[np.isfinite(member)].astype(np.float64)
    if fin.size == 0:
        return REL_L2_TOL
    p = member.astype(np.float64)
    g2 = np.zeros(p.shape)
    for ax in (0, 1):
        if p.shape[ax] > 1:
            d = np.abs(np.diff(p, axis=ax))
            d = np.where(np.isfinite(d), d, 0.0)
            pad = [(0, 0), (0, 0)]
            pad[ax] = (0, 1)
            g2 += np.pad(d, pad)
    grad = float(np.sqrt(np.mean(g2**2)))
    rms = float(np.sqrt(np.mean(fin**2)))
    mag = float(np.max(np.abs(fin)))
    if rms == 0.0:
        return REL_L2_TOL
    return min((2.0 * disp_bar * grad + _SAMPLE_ULPS * EPS32 * mag) / rms, REL_L2_TOL)


# ---- the checks --------------------------------------------------------------------------------------------------------
def _resample(member, disp, order, outval):
    """float64 map_coordinates of the member at grid + disp (mode "constant", cval=outval), with the coordinates the
    comparison must skip: within 1e-6 px of an image edge (or, for order 0, of a .5 tie) but not on it."""
    from scipy.ndimage import map_coordinates

    m, n = member.shape
    yy, xx = np.mgrid[0:m, 0:n].astype(np.float64)
    cx, cy = xx + disp[0], yy + disp[1]
    ok = np.isfinite(cx) & np.isfinite(cy)
    want = map_coordinates(member.astype(np.float64), [np.where(ok, cy, 0.0), np.where(ok, cx, 0.0)], order=order,
                           mode="constant", cval=outval)
    want = np.where(ok, want, outval)  # a lost trajectory (NaN coordinate) samples cval, like map_coordinates
    skip = np.zeros((m, n), bool)
    with np.errstate(invalid="ignore"):
        for c, ln in ((cx, n), (cy, m)):
            for edge in (0.0, ln - 1.0):
                d = np.abs(c - edge)
                skip |= (d > 0) & (d <= 1e-6)
            if order == 0:
                d = np.abs(c - np.floor(c) - 0.5)
                skip |= (d > 0) & (d <= 1e-6)
    return want, skip & ok


def _check_call(stats, got, gdisp, want, wdisp, touched, members, order, outval, disp_bar):
    """(a) trajectories, (b) resampling of the last plane, (c) every plane against the oracle's."""
    B = gdisp.shape[0]
    assert np.array_equal(np.isnan(gdisp), np.isnan(wdisp))
    stats["touched"] = max(stats.get("touched", 0), int(touched.sum()))
    assert touched.mean() < 0.1  # the tight comparison covers most trajectories
    for j in range(B):
        sane = np.all(np.isfinite(wdisp[j]) & (np.abs(wdisp[j]) < 1e6), axis=0) & ~touched[j]
        if sane.any():
            err = float(np.max(np.abs(gdisp[j][:, sane] - wdisp[j][:, sane])))
            stats["disp"] = max(stats.get("disp", 0.0), err)
            assert err < disp_bar, ("trajectory", j, err, disp_bar)
        if got is None:
            continue
        # (b) the member at the device's own positions: the blend rounds the weights (1 - f: 1/2 ulp, the products:
        # 1/2 ulp) and the three fma partial sums (1/2 ulp of at most |p|max each) - < 5 u |p|max, bar 8 u |p|max;
        # order 0 picks the same texel, so it is exact
        want_b, skip = _resample(members[j], gdisp[j], order, outval)
        last = got[j, -1]
        stats["skipped"] = max(stats.get("skipped", 0), int(skip.sum()))
        assert skip.sum() <= max(2, 1e-3 * skip.size), ("too many coordinates at an edge / a tie", int(skip.sum()))
        keep = ~skip
        assert np.array_equal(np.isnan(last[keep]), np.isnan(want_b[keep])), ("resampling NaN mask", j)
        fin = keep & np.isfinite(want_b)
        mag = float(np.max(np.abs(members[j][np.isfinite(members[j])]), initial=0.0))
        samp_bar = 0.0 if order == 0 else _SAMPLE_ULPS * EPS32 * max(mag, abs(outval) if np.isfinite(outval) else 0.0)
        if fin.any():
            err = float(np.max(np.abs(last[fin].astype(np.float64) - want_b[fin])))
            stats["sample"] = max(stats.get("sample", 0.0), err / max(mag, 1e-30))
            assert err <= samp_bar, ("resampling", j, err, samp_bar)
        # (c) every plane against the oracle, on the trajectories (a) holds to the budget
        rel_bar = _field_budget(members[j], disp_bar)
        calm = ~touched[j]
        for t in range(got.shape[1]):
            mm = nan_mismatch(got[j, t][calm], want[j, t][calm])
            stats["nan_mismatch"] = max(stats.get("nan_mismatch", 0), mm)
            assert mm <= NAN_EDGE, ("NaN mask", j, t, mm)
            r = rel_l2(got[j, t][calm], want[j, t][calm])
            stats["rel_l2"] = max(stats.get("rel_l2", 0.0), r)
            stats["rel_bar"] = max(stats.get("rel_bar", 0.0), rel_bar)
            assert r < rel_bar, ("plane", j, t, r, rel_bar)


def _run(V, members, calls, B, perts, n_iter, order, outval, sentinel=False, special=None):
    """``calls``: list of (increments, t_total, with_field).  Each route against one oracle chain."""
    orc = _Oracle(V, B, perts, n_iter, order, outval, special)
    wants = [orc.step(members if f else None, incs, tt) for incs, tt, f in calls]
    smax = max(max(incs) for incs, _, _ in calls) / (n_iter if n_iter > 1 else 1)
    for route in ROUTES:
        dev = _Device(route, V, B, perts, n_iter, order, outval)
        stats = {}
        n_sub = 1
        for (incs, tt, f), (want, wdisp, touched) in zip(calls, wants):
            got, gdisp = dev.step(members if f else None, incs, tt)
            n_sub += len(incs) * max(n_iter, 1)
            bar = _disp_budget(orc.vmax, orc.lip, smax, n_sub)
            stats["disp_bar"] = max(stats.get("disp_bar", 0.0), bar)
            assert (got is None) == (not f)
            _check_call(stats, got, gdisp, want, wdisp, touched, members, order, outval, bar)
            if sentinel:
                far = np.isfinite(wdisp) & (np.abs(wdisp) >= 1e6)
                gfar = np.abs(gdisp) > 1e6
                # a trajectory that met the sentinel stays out of every image, on the side it left on (sat_add) ...
                assert np.all(gfar[far]), ("astronomical displacements", route)
                flip = far & (np.sign(gdisp) != np.sign(wdisp))
                assert not flip.any(), ("wrapped", route, [(tuple(int(i) for i in k), float(gdisp[tuple(k)]),
                                                            float(wdisp[tuple(k)])) for k in np.argwhere(flip)[:6]])
                # ... and only such trajectories leave that far; one that took a sentinel tap at a weight near 0
                # (w 1e9 < 1e6 px) may land anywhere in both, with no common answer
                odd = gfar & ~far
                assert not np.any(odd & ~touched[:, None]), ("astronomical but never sampled the sentinel", route)
                stats["far_mismatch"] = max(stats.get("far_mismatch", 0), int(odd.sum()))
                assert odd.sum() <= 0.02 * far.sum(), (int(odd.sum()), int(far.sum()))
        _seen(dict(route=route, **stats))
    return wants


# ---- 1. hard motion ----------------------------------------------------------------------------------------------------
_FLOWS = ["vortex", "sink", "source", "jets", "fast", "out_right_down", "out_left_up", "diverging", "still_edges"]


def _flow(name, m, n):
    """The motion fields of test_semilag_gpu.py's window tests (px / step; positive: samples come from lower coordinates)."""
    y, x = np.mgrid[0:m, 0:n].astype(np.float64)
    cy, cx = (m - 1) / 2.0, (n - 1) / 2.0
    r = np.hypot(x - cx, y - cy) + 1e-9
    if name == "vortex":
        v = np.stack([-(y - cy) / 30.0, (x - cx) / 30.0])
    elif name == "sink":
        v = np.stack([(x - cx) / 40.0, (y - cy) / 40.0])
    elif name == "source":
        v = np.stack([-(x - cx) / 40.0, -(y - cy) / 40.0])
    elif name == "jets":
        v = np.stack([7.0 * np.tanh((y - cy) / 3.0), 0.5 * np.sin(x / 20.0)])
    elif name == "fast":
        v = np.stack([16.0 + 0.0 * x, -11.0 + 2.0 * np.sin(r / 25.0)])
    elif name == "out_right_down":
        v = np.stack([-23.0 - 0.01 * y, -17.0 + 0.02 * x])
    elif name == "out_left_up":
        v = np.stack([31.0 + 0.0 * x, 19.0 + 2.0 * np.sin(x / 40.0)])
    elif name == "diverging":
        v = np.stack([-(x - n / 2.0) / 6.0, -(y - m / 2.0) / 6.0])
    else:  # still_edges
        v = np.stack([3.0 * np.sin(np.pi * x / (n - 1)) ** 2, -2.0 * np.sin(np.pi * y / (m - 1)) ** 2])
        v[:, :, -1] = v[:, -1, :] = v[:, :, 0] = v[:, 0, :] = 0.0
    return v.astype(np.float32)


def _calm(m, n, r, c):
    mask = np.zeros((m, n), bool)
    mask[r, c] = True
    return mask


def _members(B, m, n, seed, nan=True):
    from tools import synth

    with np.errstate(all="ignore"):
        p = np.stack([synth.rain_field_db(m, n, seed=seed + j, sigma=2.0) for j in range(B)])
    bad = ~np.isfinite(p)  # a constant 1-pixel-wide "field" has no spread to scale by
    p[bad] = np.random.default_rng(seed).uniform(-15.0, 40.0, int(bad.sum()))
    if nan and m * n > 4:
        p[0, m // 3: m // 3 + max(1, m // 8), n // 4: n // 4 + max(1, n // 6)] = np.nan  # interior patch
        p[1, -2:, : max(1, n // 3)] = np.nan  # the last two rows: the mirrored tap of the last row
        p[1, : max(1, m // 3), -2:] = np.nan  # the last two columns
        p[B - 1, -1, -1] = np.nan  # the corner texel
    return p


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("flow", _FLOWS)
def test_members_hard_motion_vs_oracle(flow, perturb):
    """Nine hard flows, B = 5 (odd: the pair kernel's last thread column carries member 4 twice), NaN patches in the
    members (last two rows / columns included), a calm pixel, three chained calls; outval NaN or -15 (each flow
    takes both over its two cases)."""
    B, m, n = 5, 120, 200
    V = _flow(flow, m, n)
    V[:, 33, 47] = 0.0  # a calm pixel: V_par = 0 there
    members = _members(B, m, n, seed=100 + _FLOWS.index(flow))
    outval = np.nan if (_FLOWS.index(flow) + perturb) % 2 else -15.0
    perts = _perts(B) if perturb else None
    calls = [([1.0], 5.0, True), ([1.0], 10.0, True), ([0.5], 12.5, True)]
    _run(V, members, calls, B, perts, 1, 1, outval, special=_calm(m, n, 33, 47))


# ---- 2. multi-step calls -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n_iter,order", [(2, 0, 1), (2, 1, 1), (2, 2, 0), (2, 3, 1),
                                            (5, 0, 0), (5, 1, 1), (5, 2, 1), (5, 3, 1)])
def test_members_multi_step_calls_vs_oracle(T, n_iter, order):
    """T lead times per call with unequal increments and n_iter 0 .. 3: a fresh call (first increment first_scale =
    the undivided step), a displacement-only call, a resumed call (first increment from the stored position with
    scale[0] = step / n_iter)."""
    from tools import synth

    B, m, n = 3, 96, 160
    V = (1.5 * synth.true_velocity(m, n)).astype(np.float32)
    V[:, 40, 70] = 0.0
    members = _members(B, m, n, seed=300 + T)
    incs = [0.5, 1.0, 2.5, 0.75, 1.5][:T] if T == 5 else [0.5, 2.5]
    calls = [(incs, 5.0, True), ([0.75], 10.0, False), (incs, 15.0, True)]
    _run(V, members, calls, B, _perts(B, seed=T + n_iter), n_iter, order, -15.0 if n_iter % 2 else np.nan, special=_calm(m, n, 40, 70))


# ---- 3. edge shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,order", [((1, 1), 1), ((1, 77), 1), ((77, 1), 1), ((3, 64), 1), ((4, 65), 1),
                                         ((4, 65), 0), ((5, 63), 1), ((63, 65), 1), ((130, 257), 1), ((130, 257), 0)])
def test_members_edge_shapes_vs_oracle(shape, order):
    """Partial 64 x 4 tiles, n % 4 != 0 under the 8-byte row-pair loads, a last column / row on the interior / border
    switch; the flow leaves the image across every edge (away from the centre, with a swirl and a drift)."""
    m, n = shape
    B = 3
    y, x = np.mgrid[0:m, 0:n].astype(np.float64)
    cy, cx = (m - 1) / 2.0, (n - 1) / 2.0
    V = np.stack([-4.0 * np.tanh((x - cx) / 15.0) - 2.0 * np.tanh((y - cy) / 15.0) + 0.3,
                  -4.0 * np.tanh((y - cy) / 15.0) + 2.0 * np.tanh((x - cx) / 15.0) - 0.45]).astype(np.float32)
    members = _members(B, m, n, seed=500 + m + n)
    outval = np.nan if (m + n + order) % 2 else -15.0
    calls = [([1.0], 5.0, True), ([0.5, 1.5], 10.0, True), ([1.0], 15.0, False), ([2.0], 20.0, True)]
    _run(V, members, calls, B, _perts(B, seed=m * n), 1, order, outval)


# ---- 4. sentinel velocities --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sentinel", [1e20, -1e20, 1e9, -3e9])
def test_members_sentinel_velocities_vs_oracle(sentinel):
    """Finite garbage in the motion field (test_window_kernel_on_sentinel_velocities for the member kernels): a
    trajectory that samples it leaves every image for good, on the side it left on - the saturating integer adds keep
    the records from wrapping back - and the perturbation at the patch (|V|^2 overflows float32 for 1e20) is the
    float64 reference's.  Fields and sane displacements match the oracle, astronomical ones stay astronomical."""
    from tools import synth

    B, m, n = 3, 128, 192
    V = synth.true_velocity(m, n)
    V[0, 50:58, 100:112] = sentinel
    V[1, 80:90, 40:50] = -sentinel
    members = _members(B, m, n, seed=700, nan=False)
    calls = [([1.0, 1.0], 5.0, True), ([1.0], 10.0, False), ([1.0], 15.0, True), ([1.0], 20.0, True)]
    wants = _run(V, members, calls, B, _perts(B, seed=9), 1, 1, -15.0, sentinel=True, special=np.abs(V).max(axis=0) > 1e4)
    wdisp = wants[-1][1]
    insane = ~np.all(np.abs(wdisp) < 1e6, axis=1)
    assert insane.mean() < 0.1 and np.all(insane.sum(axis=(1, 2)) > 50)  # every member sampled the patches


# ---- 5. helpers --------------------------------------------------------------------------------------------------------
def test_velocity_unit_against_numpy():
    """psh_velocity_unit_dev against noise/motion.py:127-131 in float64: V / |V|, zeros at |V| <= 1e-12 and at NaN,
    and the unit vector where u^2 + v^2 overflows float32 (a 1e20 sentinel).  sqrt and the division are correctly
    rounded, u^2 + v^2 adds three roundings: <= 4 u = 4 * 2^-24."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    rng = np.random.default_rng(1)
    m, n = 37, 131
    V = (rng.standard_normal((2, m, n)) * 5).astype(np.float32)
    special = [(0.0, 0.0), (5e-13, 0.0), (0.0, -6e-13), (3e-12, 0.0), (2e-12, -2e-12), (np.nan, 1.0), (1.0, np.nan),
               (1e20, 0.0), (-1e20, 3.0), (2.0, -1e20), (1e20, 1e20), (3e38, -3e38), (1e19, 2e19), (3e9, -1e9),
               (1e-30, 0.0), (np.inf, 1.0), (-0.0, 0.0)]
    for k, (u, v) in enumerate(special):
        V[:, k // n, k % n] = (u, v)
    dv = DeviceArray.from_host(V, np.float32)
    vh = DeviceArray((2, m, n), np.float32)
    _lib.check(_lib.lib().psh_velocity_unit_dev(dv.ptr, m, n, vh.ptr))
    got = np.array(vh.to_host()).astype(np.float64)
    V64 = V.astype(np.float64)
    with np.errstate(all="ignore"):
        N = np.linalg.norm(V64, axis=0)
        want = np.where(N > 1e-12, V64 / np.where(N > 1e-12, N, 1.0), 0.0)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.all(got[~np.isfinite(want) & ~np.isnan(want)] == want[~np.isfinite(want) & ~np.isnan(want)])
    assert np.all(np.abs(got[fin] - want[fin]) <= 4 * EPS32), float(np.max(np.abs(got[fin] - want[fin])))
    assert np.all(got[want == 0.0] == 0.0)
    # the overflowing sentinels: a unit vector, as in float64
    assert got[0, 0, 7] == 1.0 and got[1, 0, 7] == 0.0
    assert np.abs(np.hypot(got[0, 0, 10], got[1, 0, 10]) - 1.0) < 4 * EPS32


def test_members_pack_against_numpy_interleave():
    """psh_members_pack_dev: {u, v, V_par_x, V_par_y} / {u, v} per pixel, bit for bit (NaNs and odd shapes included)."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    rng = np.random.default_rng(2)
    for m, n in [(1, 1), (3, 65), (130, 257)]:
        V = rng.standard_normal((2, m, n)).astype(np.float32)
        H = rng.standard_normal((2, m, n)).astype(np.float32)
        V.flat[:: 7] = np.nan
        H.flat[3:: 11] = -np.inf
        dv, dh = DeviceArray.from_host(V), DeviceArray.from_host(H)
        p4, p2 = DeviceArray((m, n, 4), np.float32), DeviceArray((m, n, 2), np.float32)
        _lib.check(_lib.lib().psh_members_pack_dev(dv.ptr, dh.ptr, m, n, p4.ptr))
        _lib.check(_lib.lib().psh_members_pack_dev(dv.ptr, None, m, n, p2.ptr))
        want4 = np.stack([V[0], V[1], H[0], H[1]], axis=-1)
        want2 = np.stack([V[0], V[1]], axis=-1)
        assert np.array_equal(np.array(p4.to_host()).view(np.uint32), want4.view(np.uint32))
        assert np.array_equal(np.array(p2.to_host()).view(np.uint32), want2.view(np.uint32))


def test_state_disp_round_trips():
    """Records -> float64 displacement -> records is bit-identical wherever the double holds P + f exactly (|P| < 2^29
    and f a multiple of 2^-24: at most 53 significant bits); a smaller fraction next to a large P is rounded by the
    double, and the records that come back are then those of the rounded displacement (NumPy model).  Displacement -> records -> displacement is exact
    against the NumPy model floor(D) + min(float32(D - floor(D)), 1 - 2^-24) wherever floor(D) fits in int32, NaN / inf
    give a lost record (NaN), and beyond int32 the integer part saturates on the side of D."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    lib = _lib.lib()
    rng = np.random.default_rng(3)
    B, m, n = 3, 5, 67
    rec = np.empty((B, m, n, 4), np.uint32)
    off = rng.integers(-(2**29) + 1, 2**29, size=(B, m, n, 2)).astype(np.int64)
    off[..., 0].flat[:40] = rng.integers(-3, 4, size=40)
    frac = (np.floor(rng.random((B, m, n, 2)) * 2.0**24) * 2.0**-24).astype(np.float32)
    frac.flat[:10] = 0.0
    frac.flat[10:20] = np.float32(1.0) - np.float32(2.0**-24)
    rec[..., :2] = off.astype(np.int32).view(np.uint32)
    rec[..., 2:] = frac.view(np.uint32)
    st = DeviceArray.from_host(rec)
    disp = DeviceArray((B, 2, m, n), np.float64)
    _lib.check(lib.psh_members_state_to_disp_dev(st.ptr, B, m, n, disp.ptr))
    d = np.array(disp.to_host())
    assert np.array_equal(d, np.moveaxis(off.astype(np.float64) + frac.astype(np.float64), -1, 1))
    back = DeviceArray((B, m, n, 4), np.uint32)
    _lib.check(lib.psh_members_disp_to_state_dev(disp.ptr, B, m, n, back.ptr))
    assert np.array_equal(np.array(back.to_host()), rec)
    # any float32 fraction: state -> disp rounds P + f to a double, disp -> state splits that double
    frac = rng.random((B, m, n, 2)).astype(np.float32)
    frac.flat[:10] = np.float32(3e-9)
    rec[..., 2:] = np.minimum(frac, np.float32(1.0) - np.float32(2.0**-24)).view(np.uint32)
    st = DeviceArray.from_host(rec)
    _lib.check(lib.psh_members_state_to_disp_dev(st.ptr, B, m, n, disp.ptr))
    _lib.check(lib.psh_members_disp_to_state_dev(disp.ptr, B, m, n, back.ptr))
    d = np.moveaxis(off.astype(np.float64) + rec[..., 2:].view(np.float32).astype(np.float64), -1, 1)
    assert np.array_equal(np.array(disp.to_host()), d)
    fl = np.floor(d)
    fr = np.minimum((d - fl).astype(np.float32), np.float32(1.0) - np.float32(2.0**-24))
    want = np.empty_like(rec)
    want[..., :2] = np.moveaxis(fl, 1, -1).astype(np.int64).astype(np.int32).view(np.uint32)
    want[..., 2:] = np.moveaxis(fr, 1, -1).view(np.uint32)
    got = np.array(back.to_host())
    assert np.array_equal(got, want)
    assert (got != rec).any()  # the rounding is real: the float64 view cannot hold every record

    # displacement -> records -> displacement
    D = rng.standard_normal((B, 2, m, n)) * 300.0
    flat = D.reshape(-1)
    flat[:12] = [-1e-9, -0.0, 0.0, 3.0, -3.0, 2.0**31 - 1.5, -(2.0**31), 1e-30, -1e-30, 7.9999999999, -2.5, 1e9]
    flat[12:20] = [np.nan, np.inf, -np.inf, 1e300, 3e9, -3e9, 1e20, -1e20]
    dd = DeviceArray.from_host(D)
    rs = DeviceArray((B, m, n, 4), np.uint32)
    _lib.check(lib.psh_members_disp_to_state_dev(dd.ptr, B, m, n, rs.ptr))
    _lib.check(lib.psh_members_state_to_disp_dev(rs.ptr, B, m, n, disp.ptr))
    got = np.array(disp.to_host())
    with np.errstate(invalid="ignore"):
        fl = np.floor(D)
        fr = np.minimum((D - fl).astype(np.float32), np.float32(1.0) - np.float32(2.0**-24)).astype(np.float64)
    fits = np.isfinite(D) & (np.abs(D) < 1e300) & (fl >= -(2.0**31)) & (fl <= 2.0**31 - 1)
    assert np.array_equal(got[fits], fl[fits] + fr[fits])
    assert np.all(np.isnan(got[~np.isfinite(D) | (np.abs(D) >= 1e300)]))
    big = np.isfinite(D) & (np.abs(D) < 1e300) & ~fits
    assert big.sum() == 4 and np.all(np.abs(got[big]) > 2.0**31 - 2) and np.all(np.sign(got[big]) == np.sign(D[big]))


# ---- 6. argument checks ------------------------------------------------------------------------------------------------
def test_member_entry_points_reject_bad_arguments():
    """Each bad argument returns its documented code before anything is launched (every buffer is sized for the call,
    so a check that failed to reject could not write out of bounds), and the library stays usable afterwards."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -6
    m, n = 4, 8

    def bufs(B, T):
        return (DeviceArray((B, m, n), np.float32).fill_bytes(0), DeviceArray((B, 2, m, n), np.float64).fill_bytes(0),
                DeviceArray((B, m, n, 4), np.uint32).fill_bytes(0), DeviceArray((B, T, m, n), np.float32))

    vel = DeviceArray.from_host(np.ones((2, m, n), np.float32))
    vhat = DeviceArray.from_host(np.full((2, m, n), 0.6, np.float32))
    packed = DeviceArray((m, n, 4), np.float32)
    _lib.check(lib.psh_members_pack_dev(vel.ptr, vhat.ptr, m, n, packed.ptr))

    def call(entry, B, T=1, n_iter=1, order=1, resume=0, with_vhat=False, scalars=True, precip=True, out=True):
        pm, disp, state, o = bufs(max(B, 1), max(T, 1))
        steps = np.ones(max(T, 1))
        par = np.zeros(max(B, 1))
        head = (pm.ptr if precip else None, vel.ptr, vhat.ptr if with_vhat else None)
        sc = (par.ctypes.data, par.ctypes.data) if scalars else (None, None)
        tail = (B, m, n, steps.ctypes.data, T, n_iter, order, 0.0)
        o_ptr = o.ptr if out else None
        if entry == "f64":
            return lib.psh_semilag_members_dev(*head, *sc, *tail, disp.ptr, resume, o_ptr)
        if entry == "state":
            return lib.psh_semilag_members_state_dev(*head, *sc, *tail, state.ptr, resume, o_ptr)
        return lib.psh_semilag_members_packed_dev(*head, packed.ptr, *sc, *tail, state.ptr, resume, o_ptr)

    for entry in ("f64", "state", "packed"):
        assert call(entry, 0) == EINVAL
        assert call(entry, 65536) == EINVAL
        assert call(entry, 2, T=0) == EINVAL
        assert call(entry, 2, T=1025) == EINVAL
        assert call(entry, 600, T=1) == EUNSUPPORTED  # T + 2 B > 1024 constants
        assert call(entry, 2, order=2) == EUNSUPPORTED
        assert call(entry, 2, n_iter=-1) == EINVAL
        assert call(entry, 2, with_vhat=True, scalars=False) == EINVAL
        assert call(entry, 2, out=False) == EINVAL
        for resume in (2, 3, -1):
            assert call(entry, 2, resume=resume) == EINVAL, (entry, resume)
            assert b"resume" in lib.psh_last_error()
        assert call(entry, 2, resume=1, with_vhat=True) == 0
    assert lib.psh_members_state_to_disp_dev(None, 1, m, n, None) == EINVAL
    st, d = DeviceArray((1, m, n, 4), np.uint32), DeviceArray((1, 2, m, n), np.float64)
    assert lib.psh_members_state_to_disp_dev(st.ptr, 0, m, n, d.ptr) == EINVAL
    assert lib.psh_members_disp_to_state_dev(d.ptr, 65536, m, n, st.ptr) == EINVAL

    # the single-field entry points: resume 0, 1 or 2 (PSH_SL_RESUME_BASE)
    p = DeviceArray.from_host(np.ones((m, n), np.float32))
    disp = DeviceArray((2, m, n), np.float64).fill_bytes(0)
    o = DeviceArray((1, m, n), np.float32)
    steps = np.ones(1)
    for resume in (3, -1, 7):
        assert lib.psh_semilag_dev(p.ptr, vel.ptr, m, n, steps.ctypes.data, 1, 1, 1, 0.0, disp.ptr, resume, o.ptr) == EINVAL
        assert b"resume" in lib.psh_last_error()
        assert lib.psh_semilag_rows_dev(p.ptr, vel.ptr, m, n, steps.ctypes.data, 1, 1, 1, 0.0, disp.ptr, resume, 1, 2,
                                        o.ptr) == EINVAL
    for resume in (0, 1, 2):
        _lib.check(lib.psh_semilag_dev(p.ptr, vel.ptr, m, n, steps.ctypes.data, 1, 1, 1, 0.0, disp.ptr, resume, o.ptr))

    # still usable: a member step after all the refusals agrees with the oracle
    from oracle import semilag as osl

    V = np.stack([np.full((m, n), 0.25), np.full((m, n), -0.5)]).astype(np.float32)
    members = np.arange(2 * m * n, dtype=np.float32).reshape(2, m, n)
    dev = _Device("f64", V, 2, None, 1, 1, np.nan)
    got, _ = dev.step(members, [1.0], 0.0)
    for j in range(2):
        want = osl.extrapolate(members[j], V, [1.0], backend="scipy")
        assert nan_mismatch(got[j, 0], want[0]) == 0 and rel_l2(got[j, 0], want[0]) < 1e-6
