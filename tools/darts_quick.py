"""Device time of a resident DARTS call (``pysteps_amd.motion.get_method("darts_hip")``), split into stages.

    python tools/darts_quick.py [size] [--frames T] [--repeat N]

Defaults: 4096^2, T = 6, the reference's default keywords.  The frames are uploaded once as a float32 DeviceArray
(the resident chain: a float32 field comes back); one warm-up call, then N timed calls.  Figures are events on the
library stream (``pysteps_amd.motion.darts.last_run_stats``): "band" (widening, rfft2 per frame, band gather and the
DFT along time), "gram" (M^H M and M^H y, copied to the host), "solve" (host SVD, wall clock), "synth" (the dense
field), "total", plus the host wall clock of the whole call.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pysteps_amd import motion  # noqa: E402
from pysteps_amd.device import DeviceArray  # noqa: E402
from pysteps_amd.motion import darts  # noqa: E402
from tools import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="?", type=int, default=4096)
ap.add_argument("--frames", type=int, default=6)
ap.add_argument("--repeat", type=int, default=5)
args = ap.parse_args()

m = args.size
frames = np.maximum(synth.steps_frames(m, m, n_frames=args.frames).astype(np.float32) + 15.0, 0.0)
frames_d = DeviceArray.from_host(frames)
fn = motion.get_method("darts_hip")
field = fn(frames_d, verbose=False)  # warm-up
stats = {k: [] for k in ("band", "gram", "solve", "synth", "total")}
wall = []
for _ in range(args.repeat):
    t0 = time.perf_counter()
    field = fn(frames_d, verbose=False)
    wall.append((time.perf_counter() - t0) * 1e3)
    for k in stats:
        stats[k].append(darts.last_run_stats[k])
out = field.to_host()
res = {"size": m, "frames": args.frames, "dtype": str(field.dtype), "wall_ms_median": float(np.median(wall)),
       "wall_ms": wall}
for k, v in stats.items():
    res[k + "_ms_median"] = float(np.median(v))
res["u_mean"], res["v_mean"] = float(out[0].mean()), float(out[1].mean())
print(json.dumps(res))
