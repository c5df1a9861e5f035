"""Golden vectors for the Lagrangian probability nowcast (``nowcasts.get_method("lagrangian_probability_hip")``),
written by the UNMODIFIED reference.

    python tools/make_golden_lagprob.py        (-> tests/golden/lagprob_reference.npz)

Runs pysteps/nowcasts/lagrangian_probability.py ``forecast`` of the reference package that ``oracle.build_ref``
prepares under oracle/_ref.  Inputs are quantised (fields to 1/4, velocities to 1/64) and stored as float32, which
holds them exactly, so that the stored inputs are the exact inputs.  Per case: precip, velocity, the keywords, the
reference's extrapolated stack (``nowcasts.extrapolation.forecast`` with the same arguments), its output, the
threshold and ``gap``.

The threshold of every case sits in the middle of the widest gap between neighbouring values of the reference's
extrapolated stack inside a quantile band: ``gap = min |extrapolated - threshold|`` over the valid pixels.  A case
whose gap is below 1e-4 of the stack's range is refused.  The device extrapolator differs from the reference's by
float32 rounding; a pixel can only change sides where that difference reaches ``gap``, which the GPU test excludes by
asserting ``gap / 2`` first.

``fft_error``: the maximum over all cases of |reference output - integer restatement of the probability stage on the
stored extrapolated stack| (tests/helpers/lagprob.py), i.e. the error of SciPy's FFT convolution; the tests' bar is
5 x this value.  Error cases store the exception type and message.  Needs the reference; never runs on the GPU machine.
"""
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lagprob_reference.npz")
MIN_GAP = 1e-4  # of the extrapolated stack's range


def q4(a):
    return (np.clip(np.round(np.asarray(a, dtype=np.float64) * 4.0), 0, 255) / 4.0).astype(np.float32)


def q64(a):
    return (np.round(np.asarray(a, dtype=np.float64) * 64.0) / 64.0).astype(np.float32)


def smooth(m, n, seed):
    """Smooth rain-like field, 0 .. about 60, quantised to 1/4."""
    db = synth.rain_field_db(m, n, seed=seed).astype(np.float64)
    return q4(np.maximum(db + 15.0, 0.0) * 1.2)


def blocks(m, n, seed, size=8):
    """Piecewise-constant field of size x size blocks with values from {0, 4, .., 40}."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 11, size=(m // size + 1, n // size + 1)) * 4.0
    return q4(np.kron(coarse, np.ones((size, size)))[:m, :n])


def uniform_velocity(m, n, u, v):
    vel = np.empty((2, m, n))
    vel[0], vel[1] = u, v
    return q64(vel)


def sheared_velocity(m, n):
    return q64(synth.true_velocity(m, n).astype(np.float64) * 0.4)


def pick_threshold(stack, q_lo, q_hi):
    """Middle of the widest gap between neighbouring distinct values of the valid pixels inside the quantile band."""
    vals = np.unique(stack[np.isfinite(stack)])
    lo, hi = np.quantile(vals, [q_lo, q_hi])
    band = vals[(vals >= lo) & (vals <= hi)]
    if band.size < 2:
        raise ValueError("no two distinct values in the band")
    k = int(np.argmax(np.diff(band)))
    return float(0.5 * (band[k] + band[k + 1]))


def main():
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from helpers import lagprob as restated
    from pysteps.nowcasts import extrapolation, lagrangian_probability

    out = {"versions": json.dumps({"numpy": np.__version__, "scipy": __import__("scipy").__version__}),
           "signature": np.array(str(inspect.signature(lagrangian_probability.forecast)))}
    cases = []
    fft_error = 0.0

    def case(name, precip, velocity, timesteps, band=(0.3, 0.7), threshold=None, **kwargs):
        nonlocal fft_error
        p64, v64 = precip.astype(np.float64), velocity.astype(np.float64)
        extrap = extrapolation.forecast(p64.copy(), v64.copy(), timesteps, kwargs.get("extrap_method", "semilagrangian"),
                                        kwargs.get("extrap_kwargs"))
        valid = np.isfinite(extrap)
        if threshold is None:
            threshold = pick_threshold(extrap, *band)
        gap = float(np.min(np.abs(extrap[valid] - threshold)))
        span = float(extrap[valid].max() - extrap[valid].min())
        if not gap > MIN_GAP * span:
            raise ValueError("%s: gap %.3g below %.3g of the range %.3g - pick another threshold" % (name, gap, MIN_GAP, span))
        res = lagrangian_probability.forecast(p64.copy(), v64.copy(), timesteps, threshold, **kwargs)
        leads = np.arange(1, timesteps + 1) if isinstance(timesteps, int) else timesteps
        scales = [int(t * kwargs.get("slope", 5)) for t in leads]
        want = restated.probability_stack(extrap, threshold, scales)
        assert np.array_equal(np.isnan(res), np.isnan(want)), name
        err = float(np.nanmax(np.abs(res - want))) if np.isfinite(want).any() else 0.0
        fft_error = max(fft_error, err)
        cases.append(name)
        out[name + "__precip"] = precip
        out[name + "__velocity"] = velocity
        out[name + "__timesteps"] = np.array(json.dumps(timesteps))
        out[name + "__kwargs"] = np.array(json.dumps(kwargs))
        out[name + "__threshold"] = np.array(threshold, dtype=np.float64)
        out[name + "__gap"] = np.array(gap, dtype=np.float64)
        out[name + "__scales"] = np.array(scales, dtype=np.int32)
        out[name + "__extrap"] = extrap
        out[name + "__out"] = res
        print("%-22s %3dx%-3d scales %-22s threshold %-8.5g gap %.3g (%.2g of range) fft error %.3g wet %.2f nan %.2f"
              % (name, precip.shape[0], precip.shape[1], scales, threshold, gap, gap / span if span else np.inf, err,
                 float(np.nanmean(extrap >= threshold)), float(np.mean(~valid))))

    # bilinear advection of smooth fields: every scale class, NaNs advected in from the border
    case("default_64x80", smooth(64, 80, 21), sheared_velocity(64, 80), 4)
    case("squares_48x64", smooth(48, 64, 22), sheared_velocity(48, 64), [0.1, 0.25, 0.5, 0.75, 1.0], slope=4)
    case("float_list_53x75", smooth(53, 75, 23), sheared_velocity(53, 75), [0.1, 0.5, 1.5, 4.0], band=(0.5, 0.8))
    case("slope1_40x52", smooth(40, 52, 24), uniform_velocity(40, 52, 1.25, -0.75), 7, slope=1, band=(0.2, 0.5))
    # NaNs in the input: a block wider than every kernel of the case (all-NaN neighbourhoods) and scattered pixels
    p = smooth(64, 80, 25)
    p[20:44, 30:58] = np.nan
    p[5, 7] = p[50, 70] = p[51, 70] = np.nan
    case("nan_input_64x80", p, uniform_velocity(64, 80, 0.5, 0.25), 3, slope=3.5)
    # exact advection: nothing moves; integer-pixel shifts with the large discs on a non-square field of odd width
    case("zero_velocity_40x52", smooth(40, 52, 26), uniform_velocity(40, 52, 0.0, 0.0), 3)
    # (integer lead times: a sum like 1.97 v + 0.03 v is an ulp away from the integer and the NaN mask of the bilinear
    # sampling would hang on that ulp)
    p = smooth(72, 99, 27)
    p[40:50, 60:80] = np.nan
    case("discs_30_60_72x99", p, uniform_velocity(72, 99, 1.0, -1.0), 2, slope=30)
    case("discs_61_91_72x99", p, uniform_velocity(72, 99, -2.0, 1.0), [2, 3], slope=30.5)
    # piecewise-constant field under a uniform sub-pixel velocity; nearest-neighbour sampling
    case("blocks_subpixel_64x80", blocks(64, 80, 28), uniform_velocity(64, 80, 0.5, 0.5), [1, 2, 3], slope=2.5)
    case("interp_order0_40x52", smooth(40, 52, 29), sheared_velocity(40, 52), 3, extrap_kwargs={"interp_order": 0})
    # nothing exceeds / everything exceeds
    case("dry_32x40", q4(np.zeros((32, 40))), uniform_velocity(32, 40, 1.5, 0.5), 2, threshold=0.5)
    case("all_wet_32x40", q4(np.full((32, 40), 8.0)), uniform_velocity(32, 40, 1.5, 0.5), 2, threshold=0.5)

    errors = []
    p, v = smooth(16, 16, 30).astype(np.float64), uniform_velocity(16, 16, 1.0, 0.0).astype(np.float64)
    for label, ts in (("float", 2.5), ("tuple", (1, 2)), ("zero", 0), ("negative", -3), ("none", None)):
        try:
            lagrangian_probability.forecast(p, v, ts, 1.0)
        except Exception as exc:  # recorded as the reference raises it
            errors.append({"label": label, "timesteps": repr(ts), "type": type(exc).__name__, "message": str(exc)})
        else:
            raise AssertionError("the reference accepted timesteps=%r" % (ts,))
    out["errors"] = np.array(json.dumps(errors))
    out["cases"] = np.array(cases)
    out["fft_error"] = np.array(fft_error, dtype=np.float64)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, fft error %.3g, %d bytes" % (OUT, len(cases), fft_error, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
