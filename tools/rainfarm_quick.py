"""Device time of RainFARM downscaling (``pysteps_amd.downscaling.rainfarm``, csrc/rainfarm.hip).

    python tools/rainfarm_quick.py [lowres side] [ds_factor] [--repeat N] [--warmup W] [--save]

Defaults: a 512^2 float64 field resident on the device at ds_factor 8 (4096^2 out), 3 warm-up calls, 20 timed calls.
Events on the library stream; median and range.  Per ``kernel_type`` None and "gaussian": the whole resident call with
``alpha`` given (``call_ms``) and its stages as the call itself times them (``last_run_stats``) - ``draw`` (the generator's
hand-over and write-back included), ``synthesis``, ``transform``, ``reduce_exp`` (standard deviation, exp, block means),
``finish`` - each beside the floor of moving its planes once at the 6.29 TB/s copy rate of the MI355X: draw 8 MN bytes,
synthesis 16 MN, transform 16 MN, reduce_exp 32 MN (the plane is read for the mean, for the deviations and for exp, and
written once), finish 16 MN.  ``table8``: ``downscale_table`` with 8 realisations of the field, "gaussian".
``kept_generator_*``: the same calls drawing from a
``DeviceRandomStates`` handle made once.  ``draw_split_host_ms``: host wall time of the draw's four steps for one plane, the device idle before each: the
generator's hand-over (``DeviceRandomStates``: ring, jump-ahead start states), the draw itself, ``sync_back`` and the
handle's release.  ``alpha_estimate_ms``: host wall time of the slope estimate on the resident field (device rfft2, download, polyfit).
``reference_256x4``: the unmodified reference's ``downscale`` of a 256^2 field at ds_factor 4 on the host, three calls
per kernel type (NumPy and SciPy run these on one thread).  Prints one JSON line and, with ``--save``, writes it to
profiles/rainfarm/rainfarm_quick_<side>x<ds>.json.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from pysteps_amd.downscaling import rainfarm  # noqa: E402
from pysteps_amd.noise.randstate import DeviceRandomStates  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, float4 copy measured on the MI355X
STAGES = ("draw", "synthesis", "transform", "reduce_exp", "finish")
FLOOR_PLANES = {"draw": 1, "synthesis": 2, "transform": 2, "reduce_exp": 4, "finish": 2}  # float64 planes moved

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=512)
ap.add_argument("ds", nargs="?", type=int, default=8)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

side, ds = args.side, args.ds
M = side * ds
report = {"lowres_side": side, "ds_factor": ds, "highres_side": M, "repeat": args.repeat, "warmup": args.warmup,
          "copy_rate_bytes_per_s": COPY_RATE}


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def lowres_field(n, seed=3):
    from helpers import rainfarm as rf

    return rf.field((n, n), seed)


def timed(fn, planes):
    for _ in range(args.warmup):
        fn()
    total, stages = [], {s: [] for s in STAGES}
    for _ in range(args.repeat):
        e0 = Event().record()
        fn()
        e1 = Event().record()
        synchronize()
        total.append(e0.elapsed_ms(e1))
        for s in STAGES:
            stages[s].append(rainfarm.last_run_stats[s])
    out = {"call_ms": spread(total)}
    for s in STAGES:
        floor = planes * FLOOR_PLANES[s] * M * M * 8 / COPY_RATE * 1e3
        out[s] = dict(spread(stages[s]), floor_ms=floor, over_floor=float(np.median(stages[s])) / floor)
    return out


field = lowres_field(side)
resident = DeviceArray.from_host(field)
rs = np.random.RandomState(1)
for kernel in (None, "gaussian"):
    report["kernel_%s" % (kernel or "none")] = timed(
        lambda: rainfarm.downscale(resident, ds, alpha=1.8, kernel_type=kernel, randstate=rs), 1)
report["table8"] = timed(
    lambda: rainfarm.downscale_table(resident, ds, n_realizations=8, alpha=1.8, kernel_type="gaussian", randstate=rs), 8)
# the same calls drawing from a DeviceRandomStates handle the caller keeps (no hand-over per call)
kept = DeviceRandomStates([rs], 8 * M * M, n_draws=64)
for kernel in (None, "gaussian"):
    report["kept_generator_kernel_%s" % (kernel or "none")] = timed(
        lambda: rainfarm.downscale(resident, ds, alpha=1.8, kernel_type=kernel, randstate=kept), 1)
report["kept_generator_table8"] = timed(
    lambda: rainfarm.downscale_table(resident, ds, n_realizations=8, alpha=1.8, kernel_type="gaussian", randstate=kept), 8)
kept.sync_back()
kept.close()

# where the draw's time goes: host wall time of its four steps, the device idle before each
split = {"create": [], "uniform": [], "sync_back": [], "close": []}
for _ in range(args.warmup + 5):
    synchronize()
    t = [time.perf_counter()]
    gen = DeviceRandomStates([rs], M * M, n_draws=1 if M * M >= rainfarm.CHUNKED_DRAW else None)
    synchronize()
    t.append(time.perf_counter())
    u = gen.uniform(0.0, 1.0, M, M)
    synchronize()
    t.append(time.perf_counter())
    gen.sync_back()
    t.append(time.perf_counter())
    gen.close()
    t.append(time.perf_counter())
    del u
    for j, key in enumerate(split):
        split[key].append((t[j + 1] - t[j]) * 1e3)
report["draw_split_host_ms"] = {k: spread(v[args.warmup:]) for k, v in split.items()}

host = []
for _ in range(5):
    t0 = time.perf_counter()
    alpha = rainfarm.estimate_alpha(resident)
    host.append((time.perf_counter() - t0) * 1e3)
report["alpha_estimate_ms"] = spread(host)
report["alpha"] = float(alpha)
sample = rainfarm.downscale(resident, ds, alpha=1.8, randstate=np.random.RandomState(2)).to_host()
report["sample_head"] = [float(v) for v in sample[0, :4]]
del sample

try:
    from oracle import build_ref

    build_ref.activate()
    from pysteps.downscaling import rainfarm as ref

    small = lowres_field(256)
    report["reference_256x4"] = {}
    for kernel in (None, "gaussian"):
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref.downscale(small, 4, alpha=1.8, kernel_type=kernel)
            times.append(time.perf_counter() - t0)
        report["reference_256x4"]["kernel_%s_s" % (kernel or "none")] = spread(times)
    dev_small = DeviceArray.from_host(small)
    for kernel in (None, "gaussian"):
        saved_m, M = M, 256 * 4
        report["reference_256x4"]["device_kernel_%s" % (kernel or "none")] = timed(
            lambda: rainfarm.downscale(dev_small, 4, alpha=1.8, kernel_type=kernel, randstate=rs), 1)["call_ms"]
        M = saved_m
except ImportError:
    report["reference_256x4"] = None

print(json.dumps(report))
if args.save:
    os.makedirs(os.path.join(ROOT, "profiles", "rainfarm"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "rainfarm", "rainfarm_quick_%dx%d.json" % (side, ds)), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
