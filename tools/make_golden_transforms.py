"""Golden vectors and bars for the transforms and unit conversions (``pysteps_amd.utils.transformation`` /
``conversion``), written by the UNMODIFIED reference.

    python tools/make_golden_transforms.py   (-> tests/golden/transforms_reference.npz, tests/golden/transforms_bars.json)

Runs pysteps/utils/transformation.py and conversion.py of the reference package that ``oracle.build_ref`` prepares under
oracle/_ref, on the CPU, over the cases of tests/helpers/transforms.py.  The npz holds the reference's outputs and
metadata (inputs come from the helper's seeds; their SHA-256 is stored).  transforms_bars.json holds, per dtype and
pass, the reference's own deviation: float32 results against the float64 evaluation of the same expression from the
same float32 input, in spacings of the float32 nearest the float64 value; float64 results against mpmath at 50 digits,
in units of 2^-52 of the exact value; SciPy's ndtri against mpmath in units of 2^-52 max(1, |exact|); and
``bar = 5 x measured``.  The Z = a R^b pass has no entry point of its own in the reference (conversion.py:262 goes on
into the dB transform), so its line is evaluated as written there.  The script asserts that the reference's inverse
Box-Cox decisions agree with the helper's outside the open band and that the band stays under NEAR_CAP.
Needs the reference and mpmath; never runs on the GPU machine.
"""
import hashlib
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def meta_json(meta):
    """Metadata without the interpolator: {key: [type name, value]}."""
    out = {}
    for k, v in meta.items():
        if k == "inqt":
            continue
        out[k] = [type(v).__name__, None if v is None else (v if isinstance(v, str) else repr(float(v)))]
    return json.dumps(out, sort_keys=True)


def main():
    import mpmath
    import scipy
    from scipy.special import ndtri

    from helpers import elementwise as ew
    from helpers import transforms as ht
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.utils import conversion as rc
    from pysteps.utils import transformation as rt

    mpmath.mp.dps = 50
    mpf = mpmath.mpf

    def exact(kind, x, p0, p1):
        x, p0 = mpf(float(x)), mpf(float(p0))
        if kind == "boxcox":
            return mpmath.log(x) if p0 == 0 else (x ** p0 - 1) / p0
        if kind == "boxcox_inverse":
            if p0 != 0 and p0 * x + 1 <= 0:  # the logarithm of a negative number is NaN to NumPy, of zero -inf
                return mpmath.nan if p0 * x + 1 < 0 else mpf(0) if p0 > 0 else mpmath.inf
            return mpmath.exp(x) if p0 == 0 else mpmath.exp(mpmath.log(p0 * x + 1) / p0)
        if kind == "z_to_rate":
            return (x / p0) ** mpf(1.0 / float(p1))
        return p0 * x ** mpf(float(p1))

    def run(case):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            if case.kind == "boxcox":
                return rt.boxcox_transform(case.R.copy(), {"transform": None}, Lambda=case.p0, threshold=case.threshold,
                                           zerovalue=case.zerovalue)[0]
            if case.kind == "boxcox_inverse":
                return rt.boxcox_transform(case.R.copy(), {"transform": "BoxCox"}, Lambda=case.p0, threshold=case.threshold,
                                           zerovalue=case.zerovalue, inverse=True)[0]
            if case.kind == "z_to_rate":
                return rc.to_rainrate(case.R.copy(), {"transform": None, "unit": "dBZ", "threshold": 1.0, "zerovalue": 0.0},
                                      zr_a=case.p0, zr_b=case.p1)[0]
            return case.p0 * case.R.copy() ** case.p1  # conversion.py:262 as written

    out = {"versions": np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__, "mpmath": mpmath.__version__}))}
    worst = {}
    ld_gap = 0.0
    for case in ht.small_cases():
        got = run(case)
        assert got.dtype == case.dtype, (case.name, got.dtype)
        out[case.name + "__out"] = got
        out[case.name + "__sha256"] = np.array(digest(case.R))
        if case.group != "continuous":
            continue
        exp = ht.expectation(case)
        kept = ~exp.zeros if case.kind != "boxcox_inverse" else ~(got == case.dtype.type(ht.INVERSE_ZERO))
        if case.dtype == np.float32:
            dev, wrong = ew.deviation(got, ht.evaluate(case.kind, case.R, case.p0, case.p1, wide=np.float64), kept)
            how = "float64 evaluation of the same expression"
        else:
            want = np.array([np.longdouble(mpmath.nstr(exact(case.kind, x, case.p0, case.p1), 30)) if k else np.longdouble(0)
                             for x, k in zip(case.R, kept)])
            dev, wrong = ht.deviation64(got, want, kept)
            gap, _ = ht.deviation64(exp.value.astype(np.float64), want, kept)
            assert gap <= 0.5 + 1e-3, (case.name, gap)  # the helper's extended evaluation rounds to the exact value's float64
            fin = kept & np.isfinite(want) & (want != 0)
            ld_gap = max(ld_gap, float(np.max(np.abs(exp.value[fin] - want[fin]) / (np.abs(want[fin]) * np.longdouble(ht.EPS)))))
            how = "mpmath at 50 digits"
        assert wrong == 0, case.name
        if dev > worst.get(case.key, (0.0, None, None))[0]:
            worst[case.key] = (dev, case.name, how)

    bars = {}
    for key, (dev, name, how) in sorted(worst.items()):
        dev = ew.stored(dev)
        bars[key] = {"measured": dev, "bar": ht.BAR_FACTOR * dev, "worst_case": name, "against": how}

    # the open band of the inverse decision, with the bars just measured
    for case in ht.small_cases():
        if case.kind != "boxcox_inverse":
            continue
        exp = ht.expectation(case, bars[case.key]["bar"])
        zeroed = out[case.name + "__out"] == case.dtype.type(ht.INVERSE_ZERO)
        assert np.array_equal(zeroed[~exp.near], exp.zeros[~exp.near]), case.name
        if case.group == "continuous":
            assert exp.near_share() <= ht.NEAR_CAP, (case.name, exp.near_share())

    # ndtri as SciPy evaluates it, over the plotting positions the transform forms
    rng = np.random.default_rng(11)
    worst_nd = (0.0, None)
    for n, a in ((4096, 0.0), (4096, 0.375), (1 << 24, 0.0), (1 << 24, 0.375)):
        ks = np.arange(1, n + 1) if n <= 4096 else np.unique(np.concatenate([np.arange(1, 400), n + 1 - np.arange(1, 400),
                                                                             rng.integers(1, n + 1, 1500)]))
        pp = ht.plotting_positions(ks, n, a)
        got = ndtri(pp)
        for p, g in zip(pp, got):
            want = mpmath.sqrt(2) * mpmath.erfinv(2 * mpf(float(p)) - 1)
            dev = float(abs(mpf(float(g)) - want) / (mpf(ht.EPS) * max(mpf(1), abs(want))))
            if dev > worst_nd[0]:
                worst_nd = (dev, "n=%d a=%s k=%d" % (n, a, int(round(p * (n + 1 - 2 * a) + a))))
    dev = ew.stored(worst_nd[0])
    bars["ndtri"] = {"measured": dev, "bar": ht.BAR_FACTOR * dev, "worst_case": worst_nd[1], "against": "mpmath at 50 digits"}

    # normal-quantile goldens
    fields = {"nq-48x64-f32": ht.rain_field((48, 64), 21, np.float32, nans=5),
              "nq-40x50-f64-continuous": ht.rain_field((40, 50), 22, np.float64, zeros=0.5, step=None, nans=3),
              "nq-16x16-half-tied": ht.rain_field((16, 16), 23, np.float32, zeros=0.5, step=None)}
    for name, x in fields.items():
        out[name + "__sha256"] = np.array(digest(x))
        for a in (0.0, 0.375):
            tag = "%s__a%s" % (name, a)
            fwd, meta = rt.NQ_transform(x.copy(), None, a=a)
            out[tag + "__forward"] = fwd
            out[tag + "__forward_meta"] = np.array(meta_json(meta))
            moved = ht.shifted(fwd)
            moved.flat[7] = -9.0  # below the table
            moved.flat[11] = 9.0  # above it
            back, meta_back = rt.NQ_transform(moved.copy(), meta, inverse=True)
            out[tag + "__inverse"] = back
            out[tag + "__inverse_meta"] = np.array(meta_json(meta_back))

    # the metadata chain through conversion: dBZ with transform "dB" -> mm/h -> mm -> dBZ
    dbz = (10.0 * np.log10(ht.reflectivities(1031, 31, np.float64))).astype(np.float32)
    dbz[::7] = -15.0
    meta = {"transform": "dB", "unit": "dBZ", "threshold": -10.0, "zerovalue": -15.0, "accutime": 5}
    out["chain__sha256"] = np.array(digest(dbz))
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        rate, m1 = rc.to_rainrate(dbz.copy(), meta)
        depth, m2 = rc.to_raindepth(rate, m1)
        refl, m3 = rc.to_reflectivity(depth, m2)
        rate316, m4 = rc.to_rainrate(dbz.copy(), meta, zr_a=316.0, zr_b=1.5)
    for tag, arr, m in (("rate", rate, m1), ("depth", depth, m2), ("refl", refl, m3), ("rate316", rate316, m4)):
        out["chain__" + tag] = arr
        out["chain__" + tag + "_meta"] = np.array(meta_json(m))

    doc = {"bar_factor": ht.BAR_FACTOR, "bars": bars,
           "units": {"f32/*": "spacing of the float32 nearest the float64 value", "f64/*": "2^-52 of the exact value",
                     "ndtri": "2^-52 max(1, |exact|)"},
           "measured_with": "pysteps.utils.transformation / conversion of the unmodified reference on the CPU over "
                            "helpers/transforms.py::small_cases; numpy %s, scipy %s, mpmath %s" % (np.__version__, scipy.__version__,
                                                                                                  mpmath.__version__),
           "helper_extended_evaluation_vs_mpmath": ew.stored(ld_gap)}
    with open(ht.BARS_JSON, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    np.savez_compressed(ht.REFERENCE_NPZ, **out)
    print(json.dumps(doc, indent=1, sort_keys=True))
    print("%s: %.1f KiB" % (ht.REFERENCE_NPZ, os.path.getsize(ht.REFERENCE_NPZ) / 1024.0))


if __name__ == "__main__":
    main()
