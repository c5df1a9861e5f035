"""Golden vectors for the ANVIL nowcast (``nowcasts.get_method("anvil_hip")``), written by the UNMODIFIED reference.

    python tools/make_golden_anvil.py        (-> tests/golden/anvil_reference.npz)

Runs pysteps/nowcasts/anvil.py ``forecast`` of the reference package that ``oracle.build_ref`` prepares under
oracle/_ref, on seeded synthetic VIL-like frames (tools/synth.py ``steps_frames`` shifted to 0 .. 60 and quantised
to 1/64, so that the stored inputs are the exact inputs), and stores inputs, keyword arguments and outputs (float32)
of every case.  It also stores intermediates of the reference's helpers on quantised planes: ``filter_gaussian``
weights, ``_moving_window_corrcoef``, ``adjust_lag2_corrcoef2``, ``_estimate_ar{1,2}_params`` and
``_r_vil_regression``.  Needs the reference; never runs on the GPU machine.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import synth  # noqa: E402


def q64(a):
    return np.round(np.asarray(a, dtype=np.float64) * 64.0) / 64.0


def frames(m, n, k, seed):
    db = synth.steps_frames(m, n, n_frames=k, seed=seed).astype(np.float64)
    return q64(np.maximum(db + 15.0, 0.0) * 1.2)


def velocity(m, n, scale=0.5):
    return q64(synth.true_velocity(m, n, dtype=np.float64) * scale)


def pack(a):
    """quantised planes as int16 counts of 1/64, NaN = -32768 (tests unpack them)"""
    a = np.asarray(a, dtype=np.float64)
    q = np.where(np.isnan(a), -32768, np.nan_to_num(a) * 64.0)
    assert np.all(np.isnan(a) | ((q == np.round(q)) & (np.abs(q) <= 32767)))
    return q.astype(np.int16)


def rainrate_for(vil, seed):
    rng = np.random.default_rng(seed)
    return q64(np.maximum(0.15 * vil + rng.normal(0.0, 0.5, vil.shape), 0.0))


def smooth_plane(m, n, seed, sigma=3.0):
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(seed)
    g = gaussian_filter(rng.standard_normal((m, n)), sigma)
    return q64(g / g.std() * 4.0)


def main():
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.cascade.bandpass_filters import filter_gaussian
    from pysteps.nowcasts import anvil
    from pysteps.timeseries import autoregression

    import scipy

    out = {"versions": json.dumps({"scipy": scipy.__version__, "numpy": np.__version__})}
    cases = []

    def case(name, vil, vel, kwargs, rainrate=None):
        kw = dict(kwargs)
        with contextlib.redirect_stdout(io.StringIO()):
            res = anvil.forecast(vil.copy(), vel.copy(), rainrate=None if rainrate is None else rainrate.copy(), **kw)
        res = np.asarray(res)
        cases.append(name)
        out[name + "__vil_q64"] = pack(vil)
        out[name + "__velocity_q64"] = pack(vel)
        if rainrate is not None:
            out[name + "__rainrate_q64"] = pack(rainrate)
        out[name + "__kwargs"] = json.dumps(kw)
        out[name + "__out"] = res.astype(np.float32)
        print("%-14s %s -> %s  nan %d  zero %d" % (name, vil.shape, res.shape, np.isnan(res).sum(), (res == 0).sum()))

    v96 = frames(96, 96, 4, 11)
    case("ar2_default", v96, velocity(96, 96), {"timesteps": 3})
    case("ar2_w10", frames(96, 128, 4, 12), velocity(96, 128), {"timesteps": 4, "ar_window_radius": 10})
    case("ar1", frames(96, 96, 3, 13), velocity(96, 96), {"timesteps": 3, "ar_order": 1, "ar_window_radius": 10})
    vr = frames(96, 96, 4, 14)
    case("rainrate", vr, velocity(96, 96), {"timesteps": 3, "ar_window_radius": 10, "r_vil_window_radius": 3},
         rainrate=rainrate_for(vr[-1], 15))
    case("no_rr_mask", frames(96, 96, 4, 16), velocity(96, 96), {"timesteps": 3, "ar_window_radius": 10,
                                                                    "apply_rainrate_mask": False})
    vn = frames(96, 96, 4, 17)
    vn[:, synth.border_nan_mask(96, 96, frac=0.15)] = np.nan
    case("nan", vn, velocity(96, 96), {"timesteps": 3, "ar_window_radius": 10})
    case("list_ts", frames(96, 96, 4, 18), velocity(96, 96), {"timesteps": [0.5, 1.0, 2.5, 3.0], "ar_window_radius": 10})
    vo = frames(75, 101, 4, 19)
    case("odd", vo, velocity(75, 101), {"timesteps": 3, "ar_window_radius": 7, "n_cascade_levels": 5},
         rainrate=rainrate_for(vo[-1], 20))
    case("norain", np.zeros((4, 100, 100)), np.zeros((2, 100, 100)), {"timesteps": 3})
    out["names"] = np.array(cases)

    # band-pass weights
    for tag, shape, nl in (("bp_64x48", (64, 48), 6), ("bp_75x101", (75, 101), 5)):
        bp = filter_gaussian(shape, nl)
        out[tag + "__w1"] = bp["weights_1d"]
        out[tag + "__w2"] = bp["weights_2d"]

    # moving-window correlations, the lag-2 adjustment, the AR parameters
    x, y1, y2 = smooth_plane(48, 64, 1), smooth_plane(48, 64, 2), smooth_plane(48, 64, 3)
    y1 = q64(0.7 * x + 0.3 * y1)
    y2 = q64(0.4 * x + 0.6 * y2)
    x[:, :6] = 0.0  # a stripe with no signal: correlation 0 there
    out["corr__x_q64"], out["corr__y1_q64"], out["corr__y2_q64"] = pack(x), pack(y1), pack(y2)
    for r in (5, 50):
        g1 = anvil._moving_window_corrcoef(x, y1, r)
        g2 = anvil._moving_window_corrcoef(x, y2, r)
        with np.errstate(all="ignore"):
            g2a = autoregression.adjust_lag2_corrcoef2(g1, g2)
            phi2 = np.stack(anvil._estimate_ar2_params(np.stack([g1, g2a]))[:3])
        phi1 = np.stack(anvil._estimate_ar1_params(g1[np.newaxis])[:2])
        out["corr_r%d__g1" % r], out["corr_r%d__g2" % r], out["corr_r%d__g2adj" % r] = g1, g2, g2a
        out["corr_r%d__phi2" % r] = phi2
        if r == 5:
            out["corr_r5__phi1"] = phi1

    # R(VIL) regression
    vil = frames(48, 64, 2, 21)[-1]
    vil[:4, :4] = np.nan
    rr = rainrate_for(np.nan_to_num(vil), 22)
    out["rvil__vil_q64"], out["rvil__rainrate_q64"] = pack(vil), pack(rr)
    with np.errstate(all="ignore"):
        a, b = anvil._r_vil_regression(vil, rr, 3)
    out["rvil__a"], out["rvil__b"] = a, b

    dst = os.path.join(ROOT, "tests", "golden", "anvil_reference.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
