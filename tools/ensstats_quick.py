"""Device time of the ensemble products (``pysteps_amd.postprocessing.ensemblestats``, csrc/ensstats.hip) and what they
save the nowcast loop.

    python tools/ensstats_quick.py [size] [--members K] [--leadtimes T] [--repeat N] [--warmup W] [--no-loop]

Defaults: 4096^2, 48 float32 members, 5 thresholds plus the mean, 3 warm-up calls, 20 timed calls, 2 lead times.

(a) ``kernel``: one fused pass over a resident stack, events on the library stream around each call, median and
    spread; the compulsory bytes (k * npix * 4 read + (1 + T) * npix * 8 written) over that time, and that rate as a
    fraction of the 6.29 TB/s float4-copy rate of the MI355X.
(b) ``loop_return_output``: the real ``pysteps.nowcasts.steps`` (oracle/_ref) through the resident loop with an
    ``EnsembleProducts`` callback and ``return_output=True``: the per-lead-time ``download`` phase of
    ``nowcasts.utils.last_run_stats`` is what every product had to wait for before this module existed.
(c) ``loop_no_output``: the same call with ``return_output=False`` - no member leaves HBM.  Loop time per lead time of
    both, from the same process.
``reference_excprob_1024``: the reference's own ``excprob`` on one thread at 1024^2 on the host; ``..._extrapolated_4096``
is that figure times 16 and is labelled as such.  Prints one JSON line and, with ``--save``, writes it to
profiles/ensstats/ensstats_quick_<size>.json.
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

from pysteps_amd import _lib  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from pysteps_amd.postprocessing import ensemblestats  # noqa: E402
from tools import synth  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, float4 copy measured on the MI355X

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="?", type=int, default=4096)
ap.add_argument("--members", type=int, default=48)
ap.add_argument("--leadtimes", type=int, default=2)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-loop", action="store_true", help="(a) only")
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m, k = args.size, args.members
thresholds = [-5.0, 0.0, 5.0, 10.0, 15.0]  # dBR
report = {"size": m, "members": k, "thresholds": thresholds, "repeat": args.repeat, "warmup": args.warmup}


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


# (a) the fused pass on a resident float32 stack: k rolled copies of a rain field in dBR with a NaN corner
field = synth.rain_field_db(m, m, seed=3).astype(np.float32)
field[: m // 16, : m // 16] = np.nan
stack = DeviceArray((k, m, m), np.float32)
for j in range(k):
    plane = DeviceArray.from_host(np.roll(field, 7 * j, axis=1) + np.float32(0.125 * (j % 5)))
    _lib.check(_lib.lib().psh_memcpy_d2d(stack.ptr + j * plane.nbytes, plane.ptr, plane.nbytes), "psh_memcpy_d2d")
synchronize()


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


npix = m * m
cases = {
    "mean_and_5_thresholds_f64_accumulate": (lambda: ensemblestats._products(stack, thresholds, True, True, True, None, True), 5, 8),
    "mean_and_5_thresholds": (lambda: ensemblestats.products(stack, thresholds, ignore_nan=True, mean_ignore_nan=True), 5, 4),
    "mean_only": (lambda: ensemblestats.mean(stack), 0, 4),
    "16_thresholds": (lambda: ensemblestats.excprob(stack, [float(t) for t in range(-8, 8)]), 16, 0),
}
report["kernel"] = {}
for name, (fn, n_thr, mean_bytes) in cases.items():
    ms = spread(timed(fn))
    nbytes = k * npix * 4 + npix * (mean_bytes + 8 * n_thr)
    rate = nbytes / (ms["median"] * 1e-3)
    report["kernel"][name] = {"ms": ms, "compulsory_bytes": nbytes, "bytes_per_s": rate, "fraction_of_copy_rate": rate / COPY_RATE}
mean_dev, probs_dev = ensemblestats._products(stack, thresholds, True, True, True, None, True)
probs = probs_dev.to_host()
report["probability_mean"] = float(np.nanmean(probs))
report["finite_fraction"] = float(np.isfinite(probs).mean())
del stack, mean_dev, probs_dev

# the reference's excprob on the host, one thread, 1024^2
try:
    from oracle import build_ref

    build_ref.activate()
    from pysteps.postprocessing import ensemblestats as ref

    small = np.stack([np.roll(field[:1024, :1024], 7 * j, axis=1) for j in range(k)]).astype(np.float64)
    t0 = time.perf_counter()
    ref.excprob(small, thresholds, ignore_nan=True)
    ref.mean(small, ignore_nan=True)
    host_s = time.perf_counter() - t0
    report["reference_products_1024_s"] = host_s
    report["reference_products_extrapolated_4096_s"] = host_s * 16.0
    del small
except ImportError:
    report["reference_products_1024_s"] = None

# (b), (c): the real nowcasts.steps through the resident loop
if not args.no_loop:
    from pysteps import nowcasts

    from pysteps_amd import register
    from pysteps_amd.nowcasts import utils as hip_loop

    from pysteps.nowcasts import steps as steps_mod

    register.register(patch_main_loop=True)
    loop_times = []
    inner = steps_mod.nowcast_main_loop

    def timed_loop(*a, **kwargs):
        # the loop alone: steps() returns no times with return_output=False, and stacks the block once more with it
        t0 = time.perf_counter()
        res = inner(*a, **kwargs)
        synchronize()
        loop_times.append(time.perf_counter() - t0)
        return res

    steps_mod.nowcast_main_loop = timed_loop
    frames = synth.steps_frames(m, m, 3)
    V = synth.true_velocity(m, m).astype(np.float64)
    kw = dict(n_ens_members=k, n_cascade_levels=6, precip_thr=-10.0, kmperpixel=1.0, timestep=5.0, seed=42, vel_pert_method="bps",
              mask_method="incremental", probmatching_method="cdf", num_workers=1,
              extrap_method="semilagrangian_hip")
    steps = nowcasts.get_method("steps")
    T = args.leadtimes
    for label, return_output in (("loop_no_output", False), ("loop_return_output", True), ("loop_no_output_again", False)):
        prod = ensemblestats.EnsembleProducts(thresholds, ignore_nan=True, mean_ignore_nan=True)
        with contextlib.redirect_stdout(io.StringIO()):
            out = steps(frames, V, T, callback=prod, return_output=return_output, **kw)
        loop_s = loop_times[-1]
        t0 = time.perf_counter()
        got = prod.excprob
        wait_s = time.perf_counter() - t0
        stats = dict(hip_loop.last_run_stats)
        report[label] = {
            "leadtimes": T, "loop_s": loop_s, "loop_s_per_leadtime": loop_s / T, "products_wait_s": wait_s,
            "phases_ms": stats, "download_ms_per_leadtime": stats.get("download", 0.0) / T,
            "callback_ms_per_leadtime": stats.get("callback", 0.0) / T, "received": sorted({c.__name__ for c in prod.received}),
            "probability_mean": float(np.nanmean(got)),
        }
        del out, got, prod

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "ensstats"), exist_ok=True)
    with open(os.path.join(root, "profiles", "ensstats", "ensstats_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
