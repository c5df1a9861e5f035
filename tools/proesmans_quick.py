"""Device time of a resident Proesmans call (``pysteps_amd.motion.get_method("proesmans_hip")``) and of its stages.

    python tools/proesmans_quick.py [side] [--iter K] [--levels L] [--warmup W] [--repeat N] [--reference MODE] [--save]

Defaults: 1024^2, the reference's default keywords (100 iterations, 6 levels), 3 warm-up and 20 timed calls, medians.
The frames (smoothed noise and the same field shifted by (1.7, -2.3) pixels) are uploaded once as a float64 DeviceArray;
the whole call is timed with events on the library stream (``pysteps_amd.motion.proesmans.last_run_stats``: "scale",
"flow", "total") next to its host wall clock.  The stages are timed one by one at the full-resolution level through the
stage functions: one pyramid level, the gradients of one frame, the consistency maps, one sweep plus edge fill, and the
step to the next level (from the half-resolution field).  ``launches_per_iteration`` counts the kernel launches of one
iteration at full resolution: three for the consistency maps, the sweep's anti-diagonals of tiles and the edge fill.

``--reference full`` times one call of the unmodified reference (oracle/_ref) on this host with the same keywords;
``--reference scaled`` times one call with 10 iterations and reports ten times that, labelled as extrapolated.
Prints one JSON line and, with ``--save``, writes it to profiles/proesmans/proesmans_quick_<side>.json.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from scipy.ndimage import gaussian_filter, shift  # noqa: E402

from pysteps_amd import _lib, motion  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from pysteps_amd.motion import proesmans as pm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=1024)
ap.add_argument("--iter", type=int, default=100)
ap.add_argument("--levels", type=int, default=6)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--reference", choices=("none", "full", "scaled"), default="none")
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m = n = args.side
base = gaussian_filter(np.random.default_rng(7).random((m + 20, n + 20)), 3.0)
base = np.where(base > 0.5, base - 0.5, 0)
frames = np.stack([base[10:10 + m, 10:10 + n], shift(base, (1.7, -2.3), order=1)[10:10 + m, 10:10 + n]])
frames_d = DeviceArray.from_host(frames)
fn = motion.get_method("proesmans_hip")
kw = dict(num_iter=args.iter, num_levels=args.levels)


def median_ms(call, warmup=2, repeat=10):
    """Median device time of ``call`` (events on the library stream)."""
    out = []
    for i in range(warmup + repeat):
        a = Event().record()
        call()
        b = Event().record()
        synchronize()
        if i >= warmup:
            out.append(a.elapsed_ms(b))
    return float(np.median(out))


for _ in range(args.warmup):
    V, gamma = fn(frames_d, full_output=True, **kw)
stats = {k: [] for k in ("scale", "flow", "total")}
wall = []
for _ in range(args.repeat):
    t0 = time.perf_counter()
    V, gamma = fn(frames_d, full_output=True, **kw)
    wall.append((time.perf_counter() - t0) * 1e3)
    for k in stats:
        stats[k].append(pm.last_run_stats[k])
res = {"side": m, "num_iter": args.iter, "num_levels": args.levels, "warmup": args.warmup, "repeat": args.repeat,
       "wall_ms_median": float(np.median(wall)), "launches_per_iteration": pm.launches_per_iteration(m, n),
       "sweep_launches_per_iteration": pm.launches_per_iteration(m, n) - 3}
for k, v in stats.items():
    res[k + "_ms_median"] = float(np.median(v))
res["per_iteration_ms"] = res["flow_ms_median"] / max(args.iter, 1)  # all levels of one iteration index

scaled, _ = pm.scale_frames(frames_d)
frame0 = scaled.view(0)
grads = DeviceArray((2, 2, m, n), np.float64)
for f in range(2):
    g = pm.gradients(scaled.view(f))
    _lib.check(_lib.lib().psh_memcpy_d2d(grads.ptr + f * g.nbytes, g.ptr, g.nbytes), "d2d")
gam = pm.consistency_maps(V)
V_half = DeviceArray((2, 2, m // 2, n // 2), np.float64).fill_bytes(0)
res["stages_ms"] = {
    "scale": median_ms(lambda: pm.scale_frames(frames_d)),
    "pyramid_level": median_ms(lambda: pm.pyramid_level(frame0)),
    "gradients_one_frame": median_ms(lambda: pm.gradients(frame0)),
    "consistency_maps": median_ms(lambda: pm.consistency_maps(V)),
    "sweep_and_edge_fill": median_ms(lambda: pm.sweep(V, gam, scaled, grads, 50.0)),
    "next_level": median_ms(lambda: pm.next_level(V_half, m, n)),
}

if args.reference != "none":
    from oracle import build_ref

    build_ref.activate()
    from pysteps.motion.proesmans import proesmans as reference

    iters = args.iter if args.reference == "full" else min(10, args.iter)
    t0 = time.perf_counter()
    reference(frames, num_iter=iters, num_levels=args.levels)
    t = time.perf_counter() - t0
    if args.reference == "full":
        res["reference_s"] = t
        res["reference_note"] = "one measured call of the unmodified reference on this host, one thread"
    else:
        res["reference_%d_iterations_s" % iters] = t
        res["reference_s_extrapolated"] = t * args.iter / iters
        res["reference_note"] = "EXTRAPOLATED: one measured call with %d iterations, scaled by %g" % (iters, args.iter / iters)

print(json.dumps(res))
if args.save:
    os.makedirs(os.path.join(ROOT, "profiles", "proesmans"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "proesmans", "proesmans_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
