"""Device time of one linear and one salient lead time of the blending (``pysteps_amd.blending``, csrc/blending.hip).

    python tools/blending_quick.py [side] [--repeat N] [--warmup W] [--save]

Defaults: 4096^2, a resident float32 nowcast and a resident float64 NWP stack, 1 and 8 members, 3 warm-up calls, 20 timed
calls, events on the library stream around each call, median and range.  ``linear_ms``: psh_blend_linear_dev with
weight 1/2; ``salient_ms``: psh_blend_salient_dev with weight 1/2, and from its own events ``prepare_ms`` (maxima, keys,
the histograms of all digits and their way to the host), ``sort_ms`` (the radix passes that are not skipped),
``distinct_ms`` (first occurrences, their scan, the compaction) and ``rank_blend_ms`` (the binary search and the blend
share one kernel: the ranks are never stored).  ``floor_ms``: reading both inputs and writing the result once at the
6.29 TB/s copy rate of the MI355X.  Prints one JSON line and, with ``--save``, writes it to
profiles/blending/blending_quick_<side>.json.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pysteps_amd import _lib  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from tools import synth  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, float4 copy measured on the MI355X
STAGES = ("prepare", "sort", "distinct", "rank_blend", "all")

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=4096)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m = args.side
plane = m * m
report = {"side": m, "repeat": args.repeat, "warmup": args.warmup, "nowcast": "float32", "nwp": "float64", "weight": 0.5}
lib = _lib.lib()


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


db = synth.rain_field_db(m, m, seed=3)
rate = np.where(db > -15.0, np.round(10.0 ** (db / 10.0) * 8.0) / 8.0, 0.0).astype(np.float32)
report["dry_share"] = float(np.mean(rate == 0))
rate[: m // 16, :] = np.nan

for K in (1, 8):
    nowcast = DeviceArray((K, 1, m, m), np.float32)
    nwp = DeviceArray((K, 1, m, m), np.float64)
    for j in range(K):
        a = DeviceArray.from_host(np.roll(rate, 5 * j, axis=1))
        b = DeviceArray.from_host(np.nan_to_num(np.roll(rate, (9, -7 * (j + 1)), axis=(0, 1))).astype(np.float64) * 1.25)
        _lib.check(lib.psh_memcpy_d2d(nowcast.ptr + j * a.nbytes, a.ptr, a.nbytes), "psh_memcpy_d2d")
        _lib.check(lib.psh_memcpy_d2d(nwp.ptr + j * b.nbytes, b.ptr, b.nbytes), "psh_memcpy_d2d")
        del a, b
    out = DeviceArray((K, 1, m, m), np.float64)
    offsets = DeviceArray.from_host(np.stack([np.arange(K, dtype=np.int64) * plane] * 3))
    synchronize()
    status = ctypes.c_int(0)
    stage = (ctypes.c_float * 5)()

    def linear():
        _lib.check(lib.psh_blend_linear_dev(nowcast.ptr, 1, nwp.ptr, 0, offsets.ptr, K, plane, 2, 0.5, 0.5, 1, out.ptr),
                   "psh_blend_linear_dev")

    def salient():
        _lib.check(lib.psh_blend_salient_dev(nowcast.ptr, 1, nwp.ptr, 0, offsets.ptr, K, plane, 0.5, 0.5, 0.25, 0.25, 1, out.ptr,
                                             ctypes.byref(status), stage), "psh_blend_salient_dev")
        assert status.value == 0

    entry = {"floor_ms": K * plane * (4 + 8 + 8) / COPY_RATE * 1e3}
    for label, fn in (("linear", linear), ("salient", salient)):
        for _ in range(args.warmup):
            fn()
        times, stages = [], []
        for _ in range(args.repeat):
            e0 = Event().record()
            fn()
            e1 = Event().record()
            synchronize()
            times.append(e0.elapsed_ms(e1))
            stages.append(list(stage))
        entry[label + "_ms"] = spread(times)
        entry[label + "_over_floor"] = entry[label + "_ms"]["median"] / entry["floor_ms"]
        if label == "salient":
            for j, name in enumerate(STAGES):
                entry[name + "_ms"] = spread([s[j] for s in stages])
    report["members_%d" % K] = entry
    del nowcast, nwp, out, offsets

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "blending"), exist_ok=True)
    with open(os.path.join(root, "profiles", "blending", "blending_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
