"""Device time of the fractions skill score (``pysteps_amd.verification.spatialscores``, csrc/fss.hip) and what the
accumulator costs the nowcast loop.

    python tools/fss_quick.py [size] [--members K] [--leadtimes T] [--repeat N] [--warmup W] [--no-loop] [--save]

Defaults: 4096^2, 48 float32 members, 5 thresholds x 8 scales, 3 warm-up calls, 20 timed calls, 2 lead times.  Events on
the library stream around each call, median and spread.

(a) ``stages``: one field, one threshold.  ``prefix_and_one_scale`` is the prefix kernel and a box pass for scale 1 (a
    window of one pixel: the cheapest box pass), ``prefix_and_eight_scales`` the prefix kernel and one box pass that
    serves 8 scales; their difference is what 7 more scales cost the box stage.  The kernels' own times come from a
    kernel trace of this script (profiles/fss/kernel_stats_<size>.txt when one was taken).
(b) ``table_k1`` and ``table_k<K>``: a 5 x 8 table for one field and for the K-member stack against a shared
    observation, beside the floor of reading the members once per threshold at the 6.29 TB/s copy rate of the MI355X.
(c) ``loop_plain`` and ``loop_with_accumulator``: the real ``pysteps.nowcasts.steps`` (oracle/_ref) through the
    resident loop with ``return_output=False``, without a callback and with an ``FssAccumulator``; the ``callback``
    phase of ``nowcasts.utils.last_run_stats`` is the accumulator's share.
``reference_fss_1024_s``: the reference's own ``fss`` for one (threshold, scale) pair at 1024^2 on the host, three
calls; ``..._extrapolated_<size>`` is the median times the area ratio and is labelled as such.  Prints one JSON line
and, with ``--save``, writes it to profiles/fss/fss_quick_<size>.json.
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
from pysteps_amd.verification import spatialscores  # noqa: E402
from tools import synth  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, float4 copy measured on the MI355X

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="?", type=int, default=4096)
ap.add_argument("--members", type=int, default=48)
ap.add_argument("--leadtimes", type=int, default=2)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-loop", action="store_true", help="(a) and (b) only")
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m, k = args.size, args.members
thresholds = [-5.0, 0.0, 5.0, 10.0, 15.0]  # dBR
scales = [1, 2, 4, 8, 16, 32, 64, 128]
report = {"size": m, "members": k, "thresholds": thresholds, "scales": scales, "repeat": args.repeat, "warmup": args.warmup}


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


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


# a resident float32 stack: k rolled copies of a rain field in dBR with a NaN corner; the observation is another roll
field = synth.rain_field_db(m, m, seed=3).astype(np.float32)
field[: m // 16, : m // 16] = np.nan
stack = DeviceArray((k, m, m), np.float32)
for j in range(k):
    plane = DeviceArray.from_host(np.roll(field, 7 * j, axis=1) + np.float32(0.125 * (j % 5)))
    _lib.check(_lib.lib().psh_memcpy_d2d(stack.ptr + j * plane.nbytes, plane.ptr, plane.nbytes), "psh_memcpy_d2d")
obs = DeviceArray.from_host(np.roll(field, (11, -5), axis=(0, 1)))
synchronize()


def sums(K, thrs, scs):
    return spatialscores._sums(stack, obs, K, m, m, True, thrs, thrs, scs)


report["stages"] = {
    "prefix_and_one_scale_ms": spread(timed(lambda: sums(1, [0.0], [1]))),
    "prefix_and_eight_scales_ms": spread(timed(lambda: sums(1, [0.0], scales))),
    "prefix_and_scale_255_ms": spread(timed(lambda: sums(1, [0.0], [255]))),
}
report["table_k1_ms"] = spread(timed(lambda: sums(1, thresholds, scales)))
table = spread(timed(lambda: sums(k, thresholds, scales)))
floor_ms = len(thresholds) * k * m * m * 4 / COPY_RATE * 1e3
report["table_k%d_ms" % k] = table
report["table_k%d_member_read_floor_ms" % k] = floor_ms
report["table_k%d_over_floor" % k] = table["median"] / floor_ms
scores = spatialscores.fss_table(stack, obs, thresholds, scales)
report["fss_mean"] = float(np.nanmean(scores))
del stack, obs

# the reference's fss on the host, one thread, one (threshold, scale) pair at 1024^2
try:
    from oracle import build_ref

    build_ref.activate()
    from pysteps.verification import spatialscores as ref

    small_f = field[:1024, :1024].astype(np.float64)
    small_o = np.roll(small_f, (11, -5), axis=(0, 1))
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref.fss(small_f, small_o, 0.0, 16)
        host.append(time.perf_counter() - t0)
    report["reference_fss_1024_s"] = spread(host)
    report["reference_fss_extrapolated_%d_s" % m] = float(np.median(host)) * (m / 1024.0) ** 2
    report["reference_table_k%d_extrapolated_%d_s" % (k, m)] = (float(np.median(host)) * (m / 1024.0) ** 2 * k * len(thresholds)
                                                                * len(scales))
except ImportError:
    report["reference_fss_1024_s"] = None

# (c): the real nowcasts.steps through the resident loop, without a callback and with the accumulator
if not args.no_loop:
    from pysteps import nowcasts
    from pysteps.nowcasts import steps as steps_mod

    from pysteps_amd import register
    from pysteps_amd.nowcasts import utils as hip_loop

    register.register(patch_main_loop=True)
    loop_times = []
    inner = steps_mod.nowcast_main_loop

    def timed_loop(*a, **kwargs):
        t0 = time.perf_counter()
        res = inner(*a, **kwargs)
        synchronize()
        loop_times.append(time.perf_counter() - t0)
        return res

    steps_mod.nowcast_main_loop = timed_loop
    frames = synth.steps_frames(m, m, 3)
    V = synth.true_velocity(m, m).astype(np.float64)
    kw = dict(n_ens_members=k, n_cascade_levels=6, precip_thr=-10.0, kmperpixel=1.0, timestep=5.0, seed=42, vel_pert_method="bps",
              mask_method="incremental", probmatching_method="cdf", num_workers=1, extrap_method="semilagrangian_hip")
    steps = nowcasts.get_method("steps")
    T = args.leadtimes
    observations = DeviceArray.from_host(np.stack([np.roll(frames[-1], (2 * (t + 1), 3 * (t + 1)), axis=(0, 1)) for t in range(T)]))
    for label, with_acc in (("loop_plain", False), ("loop_with_accumulator", True), ("loop_plain_again", False)):
        acc = spatialscores.FssAccumulator(observations, thresholds, scales) if with_acc else None
        with contextlib.redirect_stdout(io.StringIO()):
            steps(frames, V, T, callback=acc, return_output=False, **kw)
        stats = dict(hip_loop.last_run_stats)
        report[label] = {"leadtimes": T, "loop_s": loop_times[-1], "loop_s_per_leadtime": loop_times[-1] / T, "phases_ms": stats,
                         "callback_ms_per_leadtime": stats.get("callback", 0.0) / T}
        if acc is not None:
            report[label]["fss_mean"] = float(np.nanmean(acc.fss))
            report[label]["received"] = sorted({c.__name__ for c in acc.received})

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "fss"), exist_ok=True)
    with open(os.path.join(root, "profiles", "fss", "fss_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
