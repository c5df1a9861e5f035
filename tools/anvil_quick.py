"""Device time of the ANVIL nowcast (``pysteps_amd.nowcasts.get_method("anvil_hip")``), split into initialisation
and per lead time.

    python tools/anvil_quick.py [size] [--levels L] [--ar-order P] [--window R] [--timesteps T] [--repeat N]

Defaults: 4096^2, 6 cascade levels, ar_order 2, window radius 50, 12 lead times.  One warm-up call (library load,
code objects, band-pass weights uploaded and cached), then N timed calls; the figures are events on the library
stream (``pysteps_amd.nowcasts.anvil.last_run_stats``: "init" from the input upload to the last AR parameter,
"loop" the main loop) plus the host wall clock of the whole call.  Prints one JSON line.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pysteps_amd import nowcasts  # noqa: E402
from pysteps_amd.nowcasts import anvil  # noqa: E402
from tools import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="?", type=int, default=4096)
ap.add_argument("--levels", type=int, default=6)
ap.add_argument("--ar-order", type=int, default=2)
ap.add_argument("--window", type=int, default=50)
ap.add_argument("--timesteps", type=int, default=12)
ap.add_argument("--repeat", type=int, default=3)
args = ap.parse_args()

m = args.size
vil = np.maximum(synth.steps_frames(m, m, n_frames=args.ar_order + 2).astype(np.float64) + 15.0, 0.0)
vel = synth.true_velocity(m, m).astype(np.float64)
fn = nowcasts.get_method("anvil_hip")
kw = dict(timesteps=args.timesteps, n_cascade_levels=args.levels, ar_order=args.ar_order, ar_window_radius=args.window)

with contextlib.redirect_stdout(io.StringIO()):
    out = fn(vil, vel, **kw)  # warm-up
init, loop, wall = [], [], []
for _ in range(args.repeat):
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        out = fn(vil, vel, **kw)
    wall.append((time.perf_counter() - t0) * 1e3)
    init.append(anvil.last_run_stats["init"])
    loop.append(anvil.last_run_stats["loop"])
r = int(4 * args.window + 0.5)
fields = 1 + args.levels * (3 if args.ar_order == 1 else 5)
flop = fields * 2 * (3 * r + 1) * m * m  # two passes; per output: a centre product and r (add, multiply, add)
print(json.dumps({
    "size": m, "levels": args.levels, "ar_order": args.ar_order, "window": args.window, "timesteps": args.timesteps,
    "init_ms_median": float(np.median(init)), "loop_ms_median": float(np.median(loop)),
    "per_step_ms_median": float(np.median(loop)) / args.timesteps, "wall_ms_median": float(np.median(wall)),
    "init_ms": init, "loop_ms": loop, "wall_ms": wall, "filtered_fields": fields, "filter_fp64_flop": flop,
    "finite_fraction": float(np.isfinite(out).mean()), "out_mean": float(np.nanmean(out)),
}))
