"""Device time of the transforms and unit conversions on a resident field (``pysteps_amd.utils.transformation`` /
``conversion``; csrc/elementwise.hip psh_field_transform_dev, csrc/nqt.hip).

    python tools/transforms_quick.py [side] [--repeat N] [--warmup W] [--save]

Defaults: 4096^2, a resident float32 rain field with about 60 % zeros, 3 warm-up calls, 20 timed calls, events on the
library stream around each call, median and range.  Each element-wise pass stands beside ``floor_ms``: reading the input
once and writing the output once at the 6.29 TB/s copy rate of the MI355X.  The normal-quantile transform is timed stage
by stage: ``count_le`` as a whole and, from its own events, ``keys_hist`` (keys, the histograms of all digits, their way
to the host), ``sort`` (the radix passes that are not skipped) and ``counts_values`` (the upper-bound search per pixel and
the value table); then ``forward`` (ndtri per pixel, float64 result), ``table`` (the n quantiles of the inverse) and
``inverse`` (the interpolation and the two reductions).  The entry points that return a number wait for it, so their
times include that wait.  Only the search-per-pixel design of the counts exists and is measured; a sort with an index
payload and a backward scan over runs was not built, so there is no figure for it (``not_measured``).
``reference_host_1024``: the unmodified reference on one host thread at 1024^2, measured on the machine this runs on,
when the reference package is importable there (oracle/_ref); otherwise recorded as not measured.
Prints one JSON line and, with ``--save``, writes it to profiles/transforms/transforms_quick_<side>.json.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pysteps_amd import _lib, utils  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from pysteps_amd.utils import conversion  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, float4 copy measured on the MI355X

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=4096)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m = args.side
n = m * m
lib = _lib.lib()


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def rain(side, seed=3):
    rng = np.random.default_rng(seed)
    x = np.round(10.0 ** rng.uniform(-1.0, 2.0, side * side) * 8.0) / 8.0
    x[rng.random(side * side) < 0.6] = 0.0
    return x.astype(np.float32).reshape(side, side)


def timed(fn, stage=None):
    for _ in range(args.warmup):
        fn()
    times, stages = [], []
    for _ in range(args.repeat):
        e0 = Event().record()
        fn()
        e1 = Event().record()
        synchronize()
        times.append(e0.elapsed_ms(e1))
        if stage is not None:
            stages.append(list(stage))
    return times, stages


field = rain(m)
report = {"side": m, "repeat": args.repeat, "warmup": args.warmup, "dtype": "float32", "zero_share": float(np.mean(field == 0)),
          "labels": "every *_ms figure below is measured on the device of this run unless it says not_measured"}
R = DeviceArray.from_host(field)
synchronize()

floor32 = n * (4 + 4) / COPY_RATE * 1e3
meta_rate = {"transform": None, "unit": "mm/h", "threshold": 0.1, "zerovalue": 0.0, "accutime": 5}
bc, bc_meta = utils.boxcox_transform(R, meta_rate, Lambda=0.3)
lg, lg_meta = utils.boxcox_transform(R, meta_rate, Lambda=0.0)
passes = {
    "boxcox_lambda0.3": lambda: utils.boxcox_transform(R, meta_rate, Lambda=0.3),
    "boxcox_lambda0.3_inverse": lambda: utils.boxcox_transform(bc, bc_meta, inverse=True),
    "log": lambda: utils.boxcox_transform(R, meta_rate, Lambda=0.0),
    "exp": lambda: utils.boxcox_transform(lg, lg_meta, inverse=True),
    "sqrt": lambda: utils.sqrt_transform(R),
    "square": lambda: utils.sqrt_transform(R, inverse=True),
    "rate_to_z": lambda: conversion._rate_to_z(R, 200.0, 1.6),
    "z_to_rate": lambda: conversion._z_to_rate(R, 200.0, 1.6),
    "depth_to_rate": lambda: utils.to_rainrate(R, dict(meta_rate, unit="mm")),
    "rate_to_depth": lambda: utils.to_raindepth(R, meta_rate),
}
report["elementwise"] = {"floor_ms": floor32}
for name, fn in passes.items():
    times, _ = timed(fn)
    report["elementwise"][name + "_ms"] = spread(times)
    report["elementwise"][name + "_over_floor"] = float(np.median(times)) / floor32

# ---- normal-quantile transform, stage by stage ----
count = DeviceArray((m, m), np.uint32)
ordered = DeviceArray((n,), np.float32)
n_valid, lo, hi = ctypes.c_size_t(), ctypes.c_double(), ctypes.c_double()
stage = (ctypes.c_float * 3)()


def count_le():
    _lib.check(lib.psh_nqt_count_le_dev(R.ptr, 1, n, count.ptr, ordered.ptr, ctypes.byref(n_valid), ctypes.byref(lo),
                                        ctypes.byref(hi), stage), "psh_nqt_count_le_dev")


nq = {}
times, stages = timed(count_le, stage)
nq["count_le_ms"] = spread(times)
for j, name in enumerate(("keys_hist", "sort", "counts_values")):
    nq[name + "_ms"] = spread([s[j] for s in stages])
nq["count_le_floor_ms"] = n * (4 + 4 + 4) / COPY_RATE * 1e3  # the field in, the counts and the sorted values out
out64 = DeviceArray((m, m), np.float64)
thr = ctypes.c_double()
times, _ = timed(lambda: _lib.check(lib.psh_nqt_forward_dev(R.ptr, 1, count.ptr, n, n_valid.value, 0.0, 0.0, out64.ptr, 0,
                                                            ctypes.byref(thr)), "psh_nqt_forward_dev"))
nq["forward_ms"] = spread(times)
nq["forward_floor_ms"] = n * (4 + 4 + 8) / COPY_RATE * 1e3
rqn = DeviceArray((n_valid.value,), np.float64)
times, _ = timed(lambda: _lib.check(lib.psh_nqt_table_dev(n_valid.value, 0.0, rqn.ptr), "psh_nqt_table_dev"))
nq["table_ms"] = spread(times)
nq["table_floor_ms"] = n_valid.value * 8 / COPY_RATE * 1e3
back = DeviceArray((m, m), np.float64)
lowest, above = ctypes.c_double(), ctypes.c_double()
times, _ = timed(lambda: _lib.check(lib.psh_nqt_inverse_dev(out64.ptr, 0, n, rqn.ptr, ordered.ptr, 1, n_valid.value, back.ptr, 0,
                                                            ctypes.byref(lowest), ctypes.byref(above)), "psh_nqt_inverse_dev"))
nq["inverse_ms"] = spread(times)
nq["inverse_floor_ms"] = n * (8 + 8) / COPY_RATE * 1e3
times, _ = timed(lambda: utils.NQ_transform(R))
nq["NQ_transform_forward_call_ms"] = spread(times)
nq["counts_design"] = "upper-bound binary search per pixel into the sorted keys (no payload)"
nq["sort_with_index_payload_and_backward_scan_ms"] = "not_measured: this design was not built"
report["nqt"] = nq

# ---- the unmodified reference on the host at 1024^2 ----
try:
    from oracle import build_ref

    if not build_ref.available():
        raise ImportError("oracle/_ref is not built")
    build_ref.activate()
    from pysteps.utils import transformation as ref_t

    small = rain(1024)
    host = {}
    for name, fn in (("NQ_transform", lambda: ref_t.NQ_transform(small)),
                     ("boxcox_lambda0.3", lambda: ref_t.boxcox_transform(small, dict(meta_rate), Lambda=0.3)),
                     ("sqrt", lambda: ref_t.sqrt_transform(small, dict(meta_rate)))):
        fn()
        runs = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            runs.append((time.perf_counter() - t0) * 1e3)
        host[name + "_ms"] = spread(runs)
    host["note"] = "measured: host wall time of the unmodified reference, one thread, on the machine of this run"
    report["reference_host_1024"] = host
except Exception as exc:  # the reference is test infrastructure: absent on a plain installation
    report["reference_host_1024"] = "not_measured: %s" % exc

print(json.dumps(report))
if args.save:
    os.makedirs(os.path.join(ROOT, "profiles", "transforms"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "transforms", "transforms_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
