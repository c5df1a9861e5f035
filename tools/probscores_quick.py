"""Device time of the probabilistic verification scores (``pysteps_amd.verification.probscores``,
csrc/probscores.hip).

    python tools/probscores_quick.py [side] [--members K] [--repeat N] [--warmup W] [--save]

Defaults: 4096^2, 48 float32 members, 3 warm-up calls, 20 timed calls.  Events on the library stream around each call,
median and range.  ``crps_ms``: psh_crps_sums_dev of the resident stack against one observation, beside the floor of
reading the members once at the 6.29 TB/s copy rate of the MI355X (``crps_read_floor_ms``, ``crps_over_floor``).
``bins_ms``: psh_probbins_dev of one float64 probability plane, 10 bins and 10 probability thresholds, beside the floor of
reading the plane and the observation.  ``leadtime_ms``: one call of a ``ProbScoresAccumulator`` with three intensity
thresholds (CRPS, ``excprob``, three binning passes and the host arithmetic between them; wall clock included as
``leadtime_wall_ms``).  ``reference_crps_1024_s``: the unmodified reference's ``CRPS`` of the same members at 1024^2 on
one thread of the host, two calls; ``reference_crps_extrapolated_<side>_s`` is the median times the area ratio and is
labelled as such.  Prints one JSON line and, with ``--save``, writes it to
profiles/probscores/probscores_quick_<side>.json.
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
from pysteps_amd.postprocessing import ensemblestats  # noqa: E402
from pysteps_amd.verification import ProbScoresAccumulator, probscores  # noqa: E402
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
thresholds = [0.0, 5.0, 10.0]  # dBR
report = {"side": m, "members": k, "thresholds": thresholds, "repeat": args.repeat, "warmup": args.warmup}


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def timed(fn, wall=None):
    for _ in range(args.warmup):
        fn()
    times = []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        e0 = Event().record()
        fn()
        e1 = Event().record()
        synchronize()
        times.append(e0.elapsed_ms(e1))
        if wall is not None:
            wall.append((time.perf_counter() - t0) * 1e3)
    return times


def member(j, plane):
    return np.roll(plane, 7 * j, axis=1) + np.float32(0.125 * (j % 5))


field = synth.rain_field_db(m, m, seed=3).astype(np.float32)
field[: m // 16, : m // 16] = np.nan
stack = DeviceArray((k, m, m), np.float32)
for j in range(k):
    plane = DeviceArray.from_host(member(j, field))
    _lib.check(_lib.lib().psh_memcpy_d2d(stack.ptr + j * plane.nbytes, plane.ptr, plane.nbytes), "psh_memcpy_d2d")
obs_host = np.roll(field, (11, -5), axis=(0, 1))
obs = DeviceArray.from_host(obs_host)
synchronize()
npix = m * m

floor_ms = k * npix * 4 / COPY_RATE * 1e3
report["crps_read_floor_ms"] = floor_ms
t = spread(timed(lambda: probscores._crps_sums(stack, obs, 1, k, npix, True)))
report["crps_ms"] = t
report["crps_over_floor"] = t["median"] / floor_ms
report["crps"] = float(probscores.CRPS(stack, obs))

prob = ensemblestats.excprob(stack, thresholds[1])
rdiag, roc = probscores.reldiag_init(thresholds[1]), probscores.ROC_curve_init(thresholds[1])
edges, thrs = np.ascontiguousarray(rdiag["bin_edges"]), np.ascontiguousarray(roc["prob_thrs"])
bins_floor_ms = npix * (8 + 4) / COPY_RATE * 1e3
report["bins_read_floor_ms"] = bins_floor_ms
t = spread(timed(lambda: probscores._bins(prob, obs, npix, thresholds[1], edges, thrs)))
report["bins_ms"] = t
report["bins_over_floor"] = t["median"] / bins_floor_ms
del prob

wall = []
obs_stack = DeviceArray.from_host(obs_host[None])
t = spread(timed(lambda: ProbScoresAccumulator(obs_stack, thresholds)(stack), wall))
report["leadtime_ms"] = t
report["leadtime_wall_ms"] = spread(wall)
del stack, obs, obs_stack

try:
    from oracle import build_ref

    build_ref.activate()
    from pysteps.verification import probscores as ref

    small = field[:1024, :1024]
    small_f = np.stack([member(j, small) for j in range(k)])
    small_o = np.roll(small, (11, -5), axis=(0, 1))
    host = []
    for _ in range(2):
        t0 = time.perf_counter()
        ref.CRPS(small_f, small_o)
        host.append(time.perf_counter() - t0)
    report["reference_crps_1024_s"] = spread(host)
    report["reference_crps_extrapolated_%d_s" % m] = float(np.median(host)) * (m / 1024.0) ** 2
except ImportError:
    report["reference_crps_1024_s"] = None

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "probscores"), exist_ok=True)
    with open(os.path.join(root, "profiles", "probscores", "probscores_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
