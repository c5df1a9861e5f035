"""The cases on which the extrapolator's resampling is held pixel by pixel to helpers/semilag_pointwise.py on the device,
shared with the CPU tests that show the skip cap holds on them and that measure ``C_k``.  A case is a dict: name, precip (float32), velocity (float32),
timesteps (int or list) and the keyword arguments of ``extrapolate``.  Everything is deterministic.

The shapes are the smallest that reach each mechanism.  Orders 0 / 1: a 5 x 3 and two one-pixel-wide fields, one wave
with interior and border lanes (70 x 130), rows that are not 16-byte aligned (130 x 99), several tiles (257 x 131).
Orders 2 .. 5: one prefilter seam along the rows (530 x 70; segments of 512 samples), two along the columns
(70 x 1030), both axes with odd lengths (600 x 523), and a 40 x 56 control below every seam.

``python -m helpers.semilag_pointwise_cases`` (from tests/) measures ``C_k`` and rewrites
golden/semilag_pointwise_bars.json.
"""

import json

import numpy as np

from helpers import semilag_pointwise as pw

MODES = ("constant", "nearest", "reflect", "mirror", "wrap", "grid-constant", "grid-wrap")
FLOWS = ("vortex", "sink", "source", "jets", "fast", "out_of_image", "still_edges")
LOW_SHAPES = ((5, 3), (1, 37), (33, 1), (70, 130), (130, 99), (257, 131))
SPLINE_SHAPES = ((40, 56), (530, 70), (70, 1030), (600, 523))
NAN_PLACEMENTS = ("border", "last_rows_cols", "motion_hole")
SPLINE_ORDERS = (2, 3, 4, 5)


def flow(name, m, n):
    """The motion fields of test_semilag_gpu.py's window tests, scaled to the shape (px / step; positive: samples come
    from lower coordinates).  The amplitudes are not round numbers: a round velocity times a lead time puts whole rows of
    samples on, or a float32 rounding off, an image edge or a .5 tie, which is what the skip rules are for but more than
    their cap allows."""
    y, x = np.mgrid[0:m, 0:n].astype(np.float64)
    cy, cx = (m - 1) / 2.0, (n - 1) / 2.0
    half = max(cy, cx, 1.0)
    r = np.hypot(x - cx, y - cy) + 1e-9
    if name == "vortex":
        v = np.stack([-(y - cy), (x - cx)]) * (1.5 * np.pi / half)
    elif name == "sink":
        v = np.stack([(x - cx), (y - cy)]) * (np.sqrt(17.0) / half)
    elif name == "source":
        v = np.stack([-(x - cx), -(y - cy)]) * (np.sqrt(15.0) / half)
    elif name == "jets":
        v = np.stack([min(7.3, max(n, 2) / 8.13) * np.tanh((y - cy) / 3.0), 0.5 * np.sin(x / 20.0)])
    elif name == "fast":
        v = np.stack([16.0 + 0.37 * np.cos(y / 7.0), -11.0 + 2.0 * np.sin(r / 25.0)])
    elif name == "out_of_image":
        v = np.stack([-(n / 3.0 + 0.7) - 0.01 * y, -(m / 3.0 + 0.3) + 0.02 * x])
    elif name == "still_edges":
        v = np.stack([3.0 * np.sin(np.pi * x / max(n - 1, 1)) ** 2, -2.0 * np.sin(np.pi * y / max(m - 1, 1)) ** 2])
        v[:, :, -1] = v[:, -1, :] = v[:, :, 0] = v[:, 0, :] = 0.0  # exactly at rest on the edges: coordinate len - 1
    else:
        raise ValueError(name)
    return v.astype(np.float32)


def field(m, n, seed, sigma=2.0):
    from tools import synth

    with np.errstate(all="ignore"):
        p = synth.rain_field_db(m, n, seed=seed, sigma=sigma)
    bad = ~np.isfinite(p)  # a constant one-pixel-wide "field" has no spread to scale by
    p[bad] = np.random.default_rng(seed).uniform(-15.0, 40.0, int(bad.sum()))
    return p.astype(np.float32)


def _place_nans(p, v, placement):
    """-> allow_nonfinite_values.  NaNs where the border rules read them: a NaN border, the last two rows and columns
    (the mirrored tap of index len; weight 0 x NaN at coordinate len - 1), a hole in the motion field."""
    m, n = p.shape
    if placement == "border":
        if m > 2:
            p[0, :] = p[-1, :] = np.nan
        if n > 2:
            p[:, 0] = p[:, -1] = np.nan
        if m > 8 and n > 8:
            p[1, : n // 2] = p[m // 2:, 1] = np.nan  # ragged
    elif placement == "last_rows_cols":
        if m > 4:
            p[-2:, : max(1, n // 3)] = np.nan
            p[-2, n // 2:] = np.nan
        if n > 4:
            p[: max(1, m // 3), -2:] = np.nan
            p[m // 2:, -2] = np.nan
        if m > 4 and n > 4:
            p[-1, -1] = np.nan
    else:
        r0, c0 = m // 2, n // 2
        v[:, r0: r0 + max(1, m // 16), c0: c0 + max(1, n // 12)] = np.nan
        p[m // 3: m // 3 + max(1, m // 8), n // 4: n // 4 + max(1, n // 6)] = np.nan
    if not np.isfinite(p).any():
        p[m // 2, n // 2] = 1.0
    return True


def low_order_cases(order, mode):
    """Orders 0 / 1: one case per shape; flow, NaN placement, n_iter, outval, the kind of ``timesteps`` and a resumed
    displacement rotate with the shape and with (order, mode), so that each appears with every mode over the set."""
    combo = order * len(MODES) + MODES.index(mode)
    cases = []
    for i, (m, n) in enumerate(LOW_SHAPES):
        name_flow = FLOWS[(i + combo) % len(FLOWS)]
        placement = NAN_PLACEMENTS[(i + combo) % 3]
        if placement == "motion_hole" and not (mode == "constant" or (mode == "nearest" and order >= 1)):
            placement = "border"  # what a lost trajectory samples is pinned for these two modes only
        n_iter = (0, 1, 3)[(i + combo // 3) % 3]
        outval = (np.nan, -15.0, "min")[(i + combo // 2) % 3]
        v = flow(name_flow, m, n)
        p = field(m, n, seed=1000 + 10 * combo + i)
        _place_nans(p, v, placement)
        kw = dict(n_iter=n_iter, outval=outval, interp_order=order, map_coordinates_mode=mode,
                  allow_nonfinite_values=True)
        timesteps = 3 if (i + combo) % 2 else [0.5, 1.5, 2.0]
        resumed = (i + combo) % 4 == 0
        if resumed:
            yy, xx = np.mgrid[0:m, 0:n].astype(np.float64)
            prev = np.stack([-1.25 * np.nan_to_num(v[0].astype(np.float64)) + 0.3 * np.sin(yy / 7.0),
                             -0.75 * np.nan_to_num(v[1].astype(np.float64)) - 0.2 * np.cos(xx / 5.0)])
            kw["displacement_prev"] = prev
        name = "o%d-%s-%dx%d-%s-%s-K%d-%s%s%s" % (order, mode, m, n, name_flow, placement, n_iter, outval,
                                                  "" if isinstance(timesteps, int) else "-frac", "-resumed" if resumed else "")
        cases.append(dict(name=name, precip=p, velocity=v, timesteps=timesteps, kw=kw))
    return cases


def spline_cases(order, mode):
    """Orders 2 .. 5: every shape with and without NaNs; outval NaN and -15 alternate (a NaN cval of "grid-constant"
    poisons the whole prefilter, so that mode takes -15 throughout and the NaN cval in a case of its own); the motion
    carries the first 20 - 30 columns' samples out of the image (the 12-sample padding, the folded taps)."""
    from tools import synth

    combo = order * len(MODES) + MODES.index(mode)
    cases = []
    for i, (m, n) in enumerate(SPLINE_SHAPES):
        for nan in (False, True):
            p = field(m, n, seed=2000 + 10 * combo + i, sigma=3.0)
            v = (2.37 * synth.true_velocity(m, n)).astype(np.float32)
            if nan:
                p[synth.border_nan_mask(m, n, 0.1)] = np.nan
                if m > 520:
                    p[506:518, n // 3: n // 3 + 9] = np.nan  # zeroed samples across the prefilter seam at row 512
                if n > 520:
                    p[m // 3: m // 3 + 5, 508:520] = np.nan  # ... and at column 512
                p[m // 2: m // 2 + 4, n // 2: n // 2 + 6] = np.nan
                p[-2:, n // 4: n // 2] = np.nan
            outval = -15.0 if mode == "grid-constant" or (i + nan + combo) % 2 else np.nan
            kw = dict(n_iter=1, outval=outval, interp_order=order, map_coordinates_mode=mode, allow_nonfinite_values=nan)
            cases.append(dict(name="o%d-%s-%dx%d-%s-%s" % (order, mode, m, n, "nan" if nan else "finite", outval),
                              precip=p, velocity=v, timesteps=2, kw=kw))
    if mode == "grid-constant":
        m, n = SPLINE_SHAPES[0]
        p = field(m, n, seed=2900 + order, sigma=3.0)
        v = (2.37 * synth.true_velocity(m, n)).astype(np.float32)
        kw = dict(n_iter=1, outval=np.nan, interp_order=order, map_coordinates_mode=mode, allow_nonfinite_values=False)
        cases.append(dict(name="o%d-grid-constant-%dx%d-nancval" % (order, m, n), precip=p, velocity=v, timesteps=2, kw=kw))
    return cases


def xy_cases():
    """Custom ``xy_coords``: a warped grid and a half-pixel staggered one at orders 0, 1 and 3."""
    from tools import synth

    m, n = 70, 130
    yy, xx = np.mgrid[0:m, 0:n].astype(np.float64)
    grids = {"warp": np.stack([xx + 1.7 * np.sin(yy / 11.0) + 0.013 * xx, yy + 1.3 * np.cos(xx / 17.0) - 0.021 * yy]),
             "half": np.stack([xx + 0.5, yy + 0.5])}
    cases = []
    for g, (gname, xy) in enumerate(grids.items()):
        for o, order in enumerate((0, 1, 3)):
            p = field(m, n, seed=3000 + 10 * g + o)
            p[synth.border_nan_mask(m, n, 0.08)] = np.nan
            v = synth.true_velocity(m, n)
            mode = ("constant", "nearest", "reflect")[(g + o) % 3]
            kw = dict(n_iter=(1, 0, 2)[(g + o) % 3], outval=-15.0 if (g + o) % 2 else np.nan, interp_order=order,
                      map_coordinates_mode=mode, allow_nonfinite_values=True, xy_coords=xy)
            cases.append(dict(name="xy-%s-o%d-%s" % (gname, order, mode), precip=p, velocity=v,
                              timesteps=[0.5, 1.5, 2.0] if o == 1 else 2, kw=kw))
    return cases


def all_cases():
    for order in (0, 1):
        for mode in MODES:
            yield from low_order_cases(order, mode)
    for order in SPLINE_ORDERS:
        for mode in MODES:
            yield from spline_cases(order, mode)
    yield from xy_cases()


# ---- what the checks need of a case ------------------------------------------------------------------------------------
def n_leads(case):
    ts = case["timesteps"]
    return ts if isinstance(ts, int) else len(ts)


def prefix(case, k):
    ts = case["timesteps"]
    return k if isinstance(ts, int) else list(ts[:k])


def increments(case):
    ts = case["timesteps"]
    if isinstance(ts, int):
        return np.ones(ts)
    ts = np.asarray(ts, dtype=np.float64)
    return np.concatenate([ts[:1], np.diff(ts)])


def grid_off(case):
    m, n = case["precip"].shape
    return pw.grid_offsets(case["kw"].get("xy_coords"), m, n)


_DISP_CACHE = {}


def oracle_displacement(case, k):
    """The float64 oracle's displacement after the first k lead times (oracle/semilag.py, SciPy backend)."""
    from oracle import semilag as osl

    key = (case["name"], k)
    if key in _DISP_CACHE:  # the cases are deterministic functions of their names
        return _DISP_CACHE[key].copy()
    kw = case["kw"]
    with np.errstate(all="ignore"):
        _, disp = osl.extrapolate(None, case["velocity"], prefix(case, k), xy_coords=kw.get("xy_coords"),
                                  allow_nonfinite_values=True, displacement_prev=kw.get("displacement_prev"),
                                  n_iter=kw["n_iter"], return_displacement=True, backend="scipy")
    if len(_DISP_CACHE) >= 64:
        _DISP_CACHE.pop(next(iter(_DISP_CACHE)))
    _DISP_CACHE[key] = disp.copy()
    return disp


def disp_bar(case, k):
    """``_disp_budget`` of a case after k lead times (one sub-step more for the split of the start positions)."""
    v = case["velocity"].astype(np.float64)
    n_iter = case["kw"]["n_iter"]
    vmax = float(np.nanmax(np.abs(v)))
    lip = 0.0
    for ax in (1, 2):
        if v.shape[ax] > 1:
            d = np.abs(np.diff(v, axis=ax))
            if np.isfinite(d).any():
                lip = max(lip, float(np.nanmax(d)))
    smax = float(np.max(increments(case))) / (n_iter if n_iter > 1 else 1)
    return pw._disp_budget(vmax, lip, smax, 1 + k * max(n_iter, 1))


def reference_at(case, disp, bars=None):
    kw = case["kw"]
    return pw.Reference(case["precip"], disp, kw["interp_order"], kw["map_coordinates_mode"], kw["outval"],
                        grid_off(case), bars=bars)


# ---- C_k ----------------------------------------------------------------------------------------------------------------
def _contract_ulps(case):
    """The pointwise equivalent of the contract, 1e-4 x rms(field), in units of u mag for one case."""
    p = case["precip"]
    fin = p[np.isfinite(p)].astype(np.float64)
    return 1e-4 * float(np.sqrt(np.mean(fin**2))) / (pw.EPS32 * float(np.abs(fin).max()))


def measure_ck(order):
    """(C_k, the case it came from, contract): the largest deviation of the float32 restatement from the float64 SciPy
    result, in units of u mag, over the spline cases of this order at the oracle's own final displacement; and the
    smallest pointwise equivalent of the contract over the same cases, in the same units."""
    worst, where, contract = 0.0, None, np.inf
    for mode in MODES:
        for case in spline_cases(order, mode):
            kw = case["kw"]
            disp = oracle_displacement(case, n_leads(case))
            dev = pw.deviation_ulps(case["precip"], disp, order, mode, kw["outval"])
            contract = min(contract, _contract_ulps(case))
            if dev > worst:
                worst, where = dev, case["name"]
    return worst, where, contract


def stored(value):
    """A measured value as the JSON holds it: four significant digits."""
    return float("%.4g" % value)


def write_bars(path=pw.BARS_JSON):
    doc = {"unit": "u * mag, u = 2^-24, mag = the largest |p| of the zeroed field",
           "measured_with": "helpers/semilag_pointwise.py::resample_f32 against scipy.ndimage.map_coordinates in float64, "
                            "on the CPU, at the float64 oracle's displacement of helpers/semilag_pointwise_cases.py::spline_cases",
           "bar_factor": pw.BAR_FACTOR, "orders": {}}
    for order in SPLINE_ORDERS:
        ck, where, contract = measure_ck(order)
        ck = stored(ck)
        doc["orders"][str(order)] = {"C_k": ck, "bar": pw.BAR_FACTOR * ck, "worst_case": where,
                                     "contract_ulps": stored(contract)}
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return doc


if __name__ == "__main__":
    print(json.dumps(write_bars(), indent=1, sort_keys=True))
