"""Device time of the deterministic verification scores (``pysteps_amd.verification.detcatscores`` / ``detcontscores``,
csrc/detscores.hip).

    python tools/detscores_quick.py [side] [--members K] [--repeat N] [--warmup W] [--save]

Defaults: 4096^2, 48 float32 members against a shared observation, 5 thresholds, 3 warm-up calls, 20 timed calls.
Events on the library stream around each call, median and range.  ``counts_ms``: psh_detcat_counts_dev for the 5
thresholds; ``sums_ms``: psh_detcont_sums_dev; ``both_ms``: the two one after the other, what a ``DetScoresAccumulator``
queues per lead time; each beside the floor of reading the members and the observation once per kernel at the 6.29 TB/s
copy rate of the MI355X.  ``reference_*_1024_s``: the unmodified reference's ``det_cat_fct`` (one threshold) and
``det_cont_fct`` (online scores) at 1024^2 on one thread of the host, three calls; ``..._extrapolated_<side>_s`` is the
median times the area ratio and is labelled as such.  Prints one JSON line and, with ``--save``, writes it to
profiles/detscores/detscores_quick_<side>.json.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pysteps_amd import _lib  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from pysteps_amd.verification import detcatscores, detcontscores  # noqa: E402
from tools import synth  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, float4 copy measured on the MI355X

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=4096)
ap.add_argument("--members", type=int, default=48)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m, k = args.side, args.members
thresholds = [-5.0, 0.0, 5.0, 10.0, 15.0]  # dBR
report = {"side": m, "members": k, "thresholds": thresholds, "repeat": args.repeat, "warmup": args.warmup}


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def timed(fn):
    for _ in range(args.warmup):
        fn()
    times = []
    for _ in range(args.repeat):
        e0 = Event().record()
        fn()
        e1 = Event().record()
        synchronize()
        times.append(e0.elapsed_ms(e1))
    return times


field = synth.rain_field_db(m, m, seed=3).astype(np.float32)
field[: m // 16, : m // 16] = np.nan
stack = DeviceArray((k, m, m), np.float32)
for j in range(k):
    plane = DeviceArray.from_host(np.roll(field, 7 * j, axis=1) + np.float32(0.125 * (j % 5)))
    _lib.check(_lib.lib().psh_memcpy_d2d(stack.ptr + j * plane.nbytes, plane.ptr, plane.nbytes), "psh_memcpy_d2d")
obs = DeviceArray.from_host(np.roll(field, (11, -5), axis=(0, 1)))
synchronize()
npix = m * m


def counts():
    return detcatscores._counts(stack, obs, k, npix, True, thresholds, thresholds)


def sums():
    return detcontscores._sums(stack, obs, k, npix, True, 0, 0.0, 0.0)


floor_ms = (k + 1) * npix * 4 / COPY_RATE * 1e3
report["read_floor_ms"] = floor_ms
for label, fn, passes in (("counts", counts, 1), ("sums", sums, 1), ("both", lambda: (counts(), sums()), 2)):
    t = spread(timed(fn))
    report[label + "_ms"] = t
    report[label + "_over_floor"] = t["median"] / (passes * floor_ms)
report["mse_member0"] = float(detcontscores.det_cont_table(stack.view(0), obs, scores="mse")["MSE"])
del stack, obs

try:
    from oracle import build_ref

    build_ref.activate()
    from pysteps.verification import detcatscores as ref_cat
    from pysteps.verification import detcontscores as ref_cont

    small_f = field[:1024, :1024].copy()
    small_o = np.roll(small_f, (11, -5), axis=(0, 1))
    online = ["ME", "MAE", "MSE", "NMSE", "RMSE", "corr_p", "beta1", "beta2", "DRMSE", "RV"]
    for label, call in (("cat", lambda: ref_cat.det_cat_fct(small_f, small_o, 0.0)),
                        ("cont", lambda: ref_cont.det_cont_fct(small_f, small_o, online))):
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            with np.errstate(all="ignore"):
                call()
            host.append(time.perf_counter() - t0)
        report["reference_%s_1024_s" % label] = spread(host)
        report["reference_%s_extrapolated_%d_s" % (label, m)] = float(np.median(host)) * (m / 1024.0) ** 2
except ImportError:
    report["reference_cat_1024_s"] = None

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "detscores"), exist_ok=True)
    with open(os.path.join(root, "profiles", "detscores", "detscores_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
