"""Device time of the aggregation, clipping and squaring of resident fields (``pysteps_amd.utils.dimension``;
csrc/dimension.hip).

    python tools/dimension_quick.py [side] [--repeat N] [--warmup W] [--save]

Defaults: 4096^2, resident float32 rain fields with about 60 % zeros, 3 warm-up calls, 20 timed calls, events on the
library stream around each call, median and range.  Measured: the upscale by 2, 8 and 64 (the fused kernel) and by 8 as
two launches through a scratch plane; the aggregation in time of 12 planes by 12 and of a (members, 12, side, side)
stack by 6 - 48 members where 60 GB of device memory are free, else 8, recorded as ``members``; a pad and a clip of one
plane; one ``TimeAggregator`` step for 48 members (float32 members into the float64 accumulator).  Every figure stands
beside ``floor_ms``: reading the input once and writing the output once at the 6.29 TB/s copy rate of the MI355X, and the
ratio of the two.  The times are those of the public calls, so they include the allocation of the result from the block
cache and the Python around the launch.
``reference_host_1024``: the unmodified reference on one host thread at 1024^2, measured on the machine this runs on,
when the reference package is importable there (oracle/_ref); otherwise recorded as not measured.
Prints one JSON line and, with ``--save``, writes it to profiles/dimension/dimension_quick_<side>.json.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pysteps_amd import _lib  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, device_info, synchronize  # noqa: E402
from pysteps_amd.utils import dimension  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, float4 copy measured on the MI355X

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=4096)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m = args.side
lib = _lib.lib()


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def rain(rows, cols, seed=3):
    rng = np.random.default_rng(seed)
    x = np.round(10.0 ** rng.uniform(-1.0, 2.0, rows * cols) * 8.0) / 8.0
    x[rng.random(rows * cols) < 0.6] = 0.0
    return x.astype(np.float32).reshape(rows, cols)


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


def stack_of(plane_dev, shape):
    """A stack of ``shape`` whose planes are copies of one resident plane (filled on the device)."""
    out = DeviceArray(shape, plane_dev.dtype)
    for i in range(out.size // plane_dev.size):
        _lib.check(lib.psh_memcpy_d2d(out.ptr + i * plane_dev.nbytes, plane_dev.ptr, plane_dev.nbytes), "psh_memcpy_d2d")
    return out


def entry(report, name, fn, bytes_moved):
    times = timed(fn)
    floor = bytes_moved / COPY_RATE * 1e3
    report[name] = {"ms": spread(times), "floor_ms": floor, "over_floor": float(np.median(times)) / floor}


field = rain(m, m)
report = {"side": m, "repeat": args.repeat, "warmup": args.warmup, "dtype": "float32", "zero_share": float(np.mean(field == 0)),
          "copy_rate_bytes_per_s": COPY_RATE,
          "labels": "every ms figure below is measured on the device of this run unless it says not_measured"}
R = DeviceArray.from_host(field)
synchronize()
geo = {"x1": 0.0, "x2": float(m), "y1": 0.0, "y2": float(m), "xpixelsize": 1.0, "ypixelsize": 1.0, "yorigin": "upper",
       "zerovalue": 0.0, "unit": "mm/h"}
plane_bytes = m * m * 4

for w in (2, 8, 64):
    if m % w == 0:
        entry(report, "upscale_by_%d" % w, lambda w=w: dimension.aggregate_fields_space(R, geo, float(w)), plane_bytes * (1 + 1.0 / w**2))
if m % 8 == 0:
    entry(report, "upscale_by_8_two_launches", lambda: dimension._upscale_dev(R, [0, 1], [8, 8], "mean", route="two_launch"),
          plane_bytes * (1 + 1.0 / 64))
    report["upscale_by_8_two_launches"]["traffic_note"] = ("the floor is that of the fused route; the two launches also write and "
                                                            "read the (side / 8, side) scratch plane")

twelve = stack_of(R, (12, m, m))
entry(report, "time_12_planes_by_12", lambda: dimension.aggregate_fields(twelve, 12, axis=0, method="mean"), plane_bytes * 13)
members = 48 if device_info()["hbm_free"] > 60e9 else 8
report["members"] = members
ensemble = stack_of(R, (members, 12, m, m))
entry(report, "time_ensemble_12_by_6", lambda: dimension.aggregate_fields(ensemble, 6, axis=1, method="mean"),
      plane_bytes * members * 14)
del ensemble

wide = DeviceArray.from_host(rain(m - m // 4, m))
synchronize()
geo_wide = dict(geo, y2=float(m - m // 4))
entry(report, "pad_one_plane", lambda: dimension.square_domain(wide, geo_wide, method="pad"), wide.nbytes + m * m * 8)
report["pad_one_plane"]["note"] = "(3/4 side, side) float32 -> (side, side) float64; includes the minimum's reduction and its wait"
entry(report, "pad_one_plane_float32", lambda: dimension.square_domain(wide, geo_wide, method="pad", dtype=np.float32),
      wide.nbytes + m * m * 4)
quarter = m // 4
extent = (float(quarter), float(m - quarter), float(quarter), float(m - quarter))
entry(report, "clip_one_plane", lambda: dimension.clip_domain(R, geo, extent), (m // 2) ** 2 * (4 + 8))
report["clip_one_plane"]["note"] = "the inner (side / 2)^2 of a float32 plane -> float64"

stack48 = stack_of(R, (48, m, m))
agg = dimension.TimeAggregator(1 << 30, method="mean", keep="device")
agg(stack48)  # opens the window: the timed calls are additions
entry(report, "time_aggregator_step_48_members", lambda: agg(stack48), 48 * m * m * (4 + 8 + 8))
del stack48, agg

# ---- the unmodified reference on the host at 1024^2 ----
try:
    from oracle import build_ref

    if not build_ref.available():
        raise ImportError("oracle/_ref is not built")
    build_ref.activate()
    from pysteps.utils import dimension as ref_d

    s = 1024
    small = rain(s, s)
    geo_s = dict(geo, x2=float(s), y2=float(s))
    small12 = np.stack([small] * 12)
    small_wide = rain(s - s // 4, s)
    host = {}
    for name, fn in (("upscale_by_2", lambda: ref_d.aggregate_fields_space(small, geo_s, 2.0)),
                     ("upscale_by_8", lambda: ref_d.aggregate_fields_space(small, geo_s, 8.0)),
                     ("upscale_by_64", lambda: ref_d.aggregate_fields_space(small, geo_s, 64.0)),
                     ("time_12_planes_by_12", lambda: ref_d.aggregate_fields(small12, 12, axis=0, method="mean")),
                     ("pad_one_plane", lambda: ref_d.square_domain(small_wide, dict(geo_s, y2=float(s - s // 4)), method="pad")),
                     ("clip_one_plane", lambda: ref_d.clip_domain(small, geo_s, (256.0, 768.0, 256.0, 768.0)))):
        fn()
        runs = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            runs.append((time.perf_counter() - t0) * 1e3)
        host[name + "_ms"] = spread(runs)
    host["note"] = "measured: host wall time of the unmodified reference, one thread, 1024^2, on the machine of this run"
    report["reference_host_1024"] = host
except Exception as exc:  # the reference is test infrastructure: absent on a plain installation
    report["reference_host_1024"] = "not_measured: %s" % exc

print(json.dumps(report))
if args.save:
    os.makedirs(os.path.join(ROOT, "profiles", "dimension"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dimension", "dimension_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
