"""Golden vectors for the ensemble statistics (``pysteps_amd.postprocessing.ensemblestats``), written by the UNMODIFIED
reference.

    python tools/make_golden_ensstats.py        (-> tests/golden/ensstats_reference.npz)

Runs pysteps/postprocessing/ensemblestats.py ``mean`` and ``excprob`` of the reference package that ``oracle.build_ref``
prepares under oracle/_ref.  The file holds inputs and the reference's outputs only.  Per case one member stack, stored
as float32 (every value is a float32 number, so the float64 run uses the exact same numbers widened), and per dtype and
operation the reference's result: ``<case>__<dtype>__<i>`` for entry ``i`` of the JSON list ``<case>__ops``
(``{"fn", "kwargs"}``; thresholds are Python floats, as a user would write them).

Stacks: k in {1, 2, 7, 20, 48}, 48 x 80 to 97 x 131 pixels, two of them with an odd pixel count; dry pixels (zeros), a
NaN border, scattered NaN, +inf and -inf, a column that is NaN in every member, one that is infinite in every member,
and values exactly equal to a threshold - quantised ones (2.5) and float32(0.7), which is below 0.7 as a float64 and
equal to it as a float32.  Thresholds: one, three, seventeen (a second pass on the device) and a scalar.  Needs the
reference; never runs on the GPU machine.
"""
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "ensstats_reference.npz")
THREE = [0.5, 2.5, 10.0]
SEVENTEEN = [0.1, 0.25, 0.5, 0.7, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 7.5, 10.0, 15.0, 20.0, 30.0, 1e39]


def stack(k, m, n, seed):
    rng = np.random.default_rng(seed)
    base = rng.gamma(0.6, 4.0, size=(m, n))
    x = np.empty((k, m, n), dtype=np.float32)
    for j in range(k):
        wet = rng.random((m, n)) < 0.45
        x[j] = np.where(wet, np.round(base * rng.lognormal(0.0, 0.5, size=(m, n)) * 4.0) / 4.0, 0.0)
    x[rng.random(x.shape) < 0.02] = np.float32(0.7)
    x[rng.random(x.shape) < 0.02] = 2.5
    x[rng.random(x.shape) < 0.01] = np.nan
    x[rng.random(x.shape) < 0.003] = np.inf
    x[rng.random(x.shape) < 0.003] = -np.inf
    x[:, :2, :] = np.nan
    x[:, -2:, :] = np.nan
    x[:, :, :2] = np.nan
    x[:, :, -2:] = np.nan
    x[:, m // 2, n // 3] = np.nan
    x[:, m // 2, n // 3 + 1] = np.inf
    x[:, m // 2 + 1, n // 3] = -0.0
    if k > 1:
        x[0, m // 3, n // 2], x[1:, m // 3, n // 2] = np.inf, -np.inf
    return x


def main():
    import warnings

    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.postprocessing import ensemblestats as ref

    out = {"versions": json.dumps({"numpy": np.__version__}),
           "signature_mean": np.array(str(inspect.signature(ref.mean))),
           "signature_excprob": np.array(str(inspect.signature(ref.excprob)))}
    errors = []
    for fn, shape in (("mean", (5,)), ("mean", (2, 3, 4, 5)), ("excprob", (5,)), ("excprob", (4, 5))):
        try:
            getattr(ref, fn)(np.zeros(shape), *([1.0] if fn == "excprob" else []))
        except Exception as exc:  # the reference raises a bare Exception
            errors.append({"fn": fn, "shape": list(shape), "type": type(exc).__name__, "message": str(exc)})
    out["errors"] = np.array(json.dumps(errors))

    cases = []
    plan = [("k1_48x80", 1, 48, 80, True), ("k2_97x131", 2, 97, 131, False), ("k7_53x75", 7, 53, 75, True),
            ("k20_48x84", 20, 48, 84, False), ("k48_48x80", 48, 48, 80, False)]
    for seed, (name, k, m, n, long_list) in enumerate(plan):
        x32 = stack(k, m, n, seed + 11)
        ops = [{"fn": "mean", "kwargs": {}}, {"fn": "mean", "kwargs": {"ignore_nan": True}},
               {"fn": "mean", "kwargs": {"X_thr": 0.7}}, {"fn": "mean", "kwargs": {"ignore_nan": True, "X_thr": 2.5}}]
        for ignore_nan in (False, True):
            ops.append({"fn": "excprob", "kwargs": {"X_thr": [0.7], "ignore_nan": ignore_nan}})
            ops.append({"fn": "excprob", "kwargs": {"X_thr": THREE, "ignore_nan": ignore_nan}})
            ops.append({"fn": "excprob", "kwargs": {"X_thr": 2.5, "ignore_nan": ignore_nan}})
            if long_list:
                ops.append({"fn": "excprob", "kwargs": {"X_thr": SEVENTEEN, "ignore_nan": ignore_nan}})
        cases.append(name)
        out[name + "__X"] = x32
        out[name + "__ops"] = np.array(json.dumps(ops))
        for dtype in ("float32", "float64"):
            x = x32.astype(dtype)
            for i, op in enumerate(ops):
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    res = getattr(ref, op["fn"])(x.copy(), **op["kwargs"])
                out["%s__%s__%d" % (name, dtype, i)] = res
    out["cases"] = np.array(cases)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %.1f KiB" % (OUT, len(cases), os.path.getsize(OUT) / 1024.0))


if __name__ == "__main__":
    main()
