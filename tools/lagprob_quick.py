"""Device time of the Lagrangian probability nowcast (``pysteps_amd.nowcasts.get_method("lagrangian_probability_hip")``)
on resident inputs, split into the extrapolation and the probability stage.

    python tools/lagprob_quick.py [size] [--timesteps T] [--slope S] [--repeat N] [--warmup W]

Defaults: 4096^2, 12 lead times, slope 5 (disc diameters 5 .. 60), 2 warm-up calls, 7 timed calls.  The inputs are
float32 DeviceArrays and the result stays on the device, so the figures are kernel time: events on the library stream
around the two stages (``pysteps_amd.nowcasts.lagrangian_probability.last_run_stats``), median of the timed calls, and
per lead time.  ``stage_ms_by_scale`` times the probability stage alone, one plane at a time, per disc diameter.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pysteps_amd import nowcasts  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from pysteps_amd.nowcasts import lagrangian_probability as lp  # noqa: E402
from tools import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="?", type=int, default=4096)
ap.add_argument("--timesteps", type=int, default=12)
ap.add_argument("--slope", type=float, default=5)
ap.add_argument("--repeat", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

m = args.size
slope = int(args.slope) if float(args.slope).is_integer() else args.slope
precip = DeviceArray.from_host(synth.rain_field_db(m, m, seed=3).astype(np.float32))
vel = DeviceArray.from_host(synth.true_velocity(m, m).astype(np.float32))
threshold = -5.0  # dB: about a fifth of the field exceeds it
fn = nowcasts.get_method("lagrangian_probability_hip")

for _ in range(args.warmup):
    out = fn(precip, vel, args.timesteps, threshold, slope=slope)
extrap, prob, wall = [], [], []
for _ in range(args.repeat):
    synchronize()
    t0 = time.perf_counter()
    out = fn(precip, vel, args.timesteps, threshold, slope=slope)
    wall.append((time.perf_counter() - t0) * 1e3)
    extrap.append(lp.last_run_stats["extrapolation"])
    prob.append(lp.last_run_stats["probability"])

# the probability stage alone, per disc diameter: one plane of the advected stack at a time
advected = nowcasts.get_method("extrapolation")(precip, vel, 1)
by_scale = {}
for scale in sorted({int(t * slope) for t in range(1, args.timesteps + 1)}):
    lp.probability_stage(advected, threshold, [scale])
    times = []
    for _ in range(args.repeat):
        e0 = Event().record()
        lp.probability_stage(advected, threshold, [scale])
        e1 = Event().record()
        synchronize()
        times.append(e0.elapsed_ms(e1))
    by_scale[str(scale)] = float(np.median(times))

host = out.to_host()
T = args.timesteps
print(json.dumps({
    "size": m, "timesteps": T, "slope": slope, "threshold": threshold, "repeat": args.repeat, "warmup": args.warmup,
    "extrapolation_ms_median": float(np.median(extrap)), "probability_ms_median": float(np.median(prob)),
    "extrapolation_ms_per_lead": float(np.median(extrap)) / T, "probability_ms_per_lead": float(np.median(prob)) / T,
    "wall_ms_median": float(np.median(wall)), "extrapolation_ms": extrap, "probability_ms": prob, "wall_ms": wall,
    "stage_ms_by_scale": by_scale,
    "finite_fraction": float(np.isfinite(host).mean()), "out_mean": float(np.nanmean(host)),
}))
