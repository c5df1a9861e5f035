"""Golden vectors for RainFARM downscaling (``downscaling.get_method("rainfarm_hip")``), written by the UNMODIFIED reference.

    python tools/make_golden_rainfarm.py        (-> tests/golden/rainfarm_reference.npz)

Runs pysteps/downscaling/rainfarm.py ``downscale`` of the reference package that ``oracle.build_ref`` prepares under
oracle/_ref on the seeded fields of tests/helpers/rainfarm.py ``CASES`` and stores per case: the low-resolution field,
the seed (the tests redraw the uniforms from ``RandomState(seed)``), the arguments, the reference's ``alpha``, its output
without a threshold (outputs above 64 x 128 pixels on every 3rd or 7th row and column) and ``g = max |noise / std|``.
Also: the three ``ValueError`` texts, the exception type of an all-dry field with ``alpha=None``, and the four bars -
each one number, the maximum over the cases, of the reference's own deviation from the long-double restatement
(tests/helpers/rainfarm.py):

* ``deviation_noise``  its float64 noise field, in ``u = 2^-53 rms`` per pixel (helpers/fft_pointwise.py);
* ``deviation_finish`` its finish stage on a given noise field (``_compute_noise_field`` wrapped to return it),
  largest absolute difference over the case's largest output value;
* ``deviation_field``  its whole output, scaled alike;
* ``deviation_alpha``  its ``alpha`` against the long-double estimate, or its shift when ``fft2`` is the float64 chirp-z
  restatement of helpers/fft_pointwise.py, whichever is larger.

Needs the reference; never runs on the GPU machine.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "rainfarm_reference.npz")


def generate():
    from helpers import fft_pointwise as fp
    from helpers import rainfarm as rf
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.downscaling import rainfarm as ref

    out = {"versions": np.array(json.dumps({"numpy": np.__version__}))}
    messages = {}
    for key, call in (("nonfinite", lambda: ref.downscale(np.array([[1.0, np.nan], [0.0, 2.0]]), 2)),
                      ("ds_factor", lambda: ref.downscale(np.ones((4, 4)), 0)),
                      ("kernel_type", lambda: ref.downscale(rf.field((4, 4), 1) + 1.0, 2, alpha=1.0, kernel_type="box"))):
        state = np.random.get_state()
        try:
            call()
            raise AssertionError("the reference raised nothing for " + key)
        except ValueError as exc:
            messages[key] = str(exc)
        np.random.set_state(state)
    out["messages"] = np.array(json.dumps(messages))
    try:
        with np.errstate(all="ignore"):
            ref.downscale(np.zeros((8, 8)), 2)
        raise AssertionError("the reference raised nothing for an all-dry field")
    except Exception as exc:  # noqa: BLE001
        out["dry_exception"] = np.array(type(exc).__name__)

    dev = {"noise": 0.0, "finish": 0.0, "field": 0.0, "alpha": 0.0}
    own_noise = ref._compute_noise_field
    kept = {}
    for name, shape, ds, kernel, alpha, seed in rf.CASES:
        precip = rf.field(shape, seed)
        hi = (shape[0] * ds, shape[1] * ds)
        state = np.random.get_state()
        np.random.seed(seed)
        with np.errstate(all="ignore"):
            got, ref_alpha = ref.downscale(precip.copy(), ds, alpha=alpha, return_alpha=True, kernel_type=kernel)
        np.random.set_state(state)
        u = rf.draw(seed, hi)
        noise64 = rf.noise_field(u, ref_alpha, shape, ds)
        noise_ld = rf.noise_field(u, ref_alpha, shape, ds, np.longdouble)
        dev["noise"] = max(dev["noise"], fp.compare(noise64, noise_ld)[0])
        field_ld, _ = rf.finish(precip, noise_ld, ds, kernel, np.longdouble)
        dev["field"] = max(dev["field"], rf.scaled_diff(got, field_ld))
        # the finish stage alone: the reference run on a given (float64) noise field
        ref._compute_noise_field = lambda freq, a, given=noise64: given.copy()
        try:
            with np.errstate(all="ignore"):
                fin = ref.downscale(precip.copy(), ds, alpha=float(ref_alpha), kernel_type=kernel)
        finally:
            ref._compute_noise_field = own_noise
        fin_ld, g = rf.finish(precip, noise64.astype(np.longdouble), ds, kernel, np.longdouble)
        dev["finish"] = max(dev["finish"], rf.scaled_diff(fin, fin_ld))
        if alpha is None:
            a_ld = rf.estimate_alpha(precip, dtype=np.longdouble)
            a_chirp = rf.estimate_alpha(precip, fft2=lambda x: fp.restated("fft2", x, x.shape))
            dev["alpha"] = max(dev["alpha"], abs(float(ref_alpha) - a_ld), abs(float(ref_alpha) - a_chirp))
        stride = rf.stride_for(hi)
        out[name + "__precip"] = precip
        out[name + "__seed"] = np.array(seed)
        out[name + "__ds"] = np.array(ds)
        out[name + "__kernel"] = np.array(kernel or "")
        out[name + "__alpha_arg"] = np.array(np.nan if alpha is None else alpha)
        out[name + "__alpha"] = np.array(float(ref_alpha))
        out[name + "__stride"] = np.array(stride)
        out[name + "__out"] = np.ascontiguousarray(got[::stride, ::stride])
        out[name + "__g"] = np.array(g)
        if name in rf.THRESHOLD_CASES:
            kept[name] = (got, g, hi)
    for key, value in dev.items():
        out["deviation_" + key] = np.array(value)
    out["cases"] = np.array([c[0] for c in rf.CASES])
    # the thresholds the tests use must not sit inside the bar of more than 0.1 % of a case's pixels
    bars = fp.load_bars()
    for name, (got, g, hi) in kept.items():
        B = fp.bar(bars, fp.shape_class(hi), "irfft2")
        bar = (rf.BAR_FACTOR * dev["field"] + 2 * (1 + g) * B * 2.0 ** -53) * np.abs(got).max()
        for thr in (0.1, float(np.median(got[got > 0]))):
            near = np.count_nonzero(np.abs(got - thr) <= bar)
            assert near <= rf.THRESHOLD_SKIP_SHARE * got.size, (name, thr, near)
    return out


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %d bytes" % (OUT, len(out["cases"]), os.path.getsize(OUT)))
    print({k: float(out[k]) for k in out if k.startswith("deviation_")})


if __name__ == "__main__":
    main()
