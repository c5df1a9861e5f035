"""Device time of the radially averaged power spectrum (``pysteps_amd.utils.spectral``, csrc/rapsd.hip).

    python tools/rapsd_quick.py [side] [--members K] [--repeat N] [--warmup W] [--save]

Defaults: 4096^2, 48 float32 members, 3 warm-up calls, 20 timed calls.  Events on the library stream around each call,
median and range.  ``binning_ms``: psh_rapsd_half_dev alone on one resident half spectrum, beside the floor of reading
that spectrum once at the 6.29 TB/s copy rate of the MI355X; ``counts_ms``: psh_rapsd_counts_dev alone (the same kernel every
binning call launches ahead of its sums); ``rfft2_ms``: psh_fft_rfft2_dev alone on the resident
float64 field; ``rapsd_ms``: ``rapsd(field, fft_method="hip")`` of that field, with its finiteness scan and the download
of the ``nb`` means; ``table_ms``: ``rapsd_table`` of the resident float32 members.  ``reference_1024_s``: the
unmodified reference's ``rapsd(field, fft_method=np.fft)`` at 1024^2 on the host, three calls;
``reference_extrapolated_<side>_s`` is the median times the ratio of ``area * bins`` (the reference passes over the
plane once per radius) and is labelled as such.  Prints one JSON line and, with ``--save``, writes it to
profiles/rapsd/rapsd_quick_<side>.json.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pysteps_amd import _lib  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from pysteps_amd.utils import spectral  # noqa: E402
from tools import synth  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s, float4 copy measured on the MI355X

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=4096)
ap.add_argument("--members", type=int, default=48)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m, k = args.side, args.members
nh, nb = m // 2 + 1, spectral._bins(m, m)
report = {"side": m, "members": k, "bins": nb, "repeat": args.repeat, "warmup": args.warmup}


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


field = np.nan_to_num(synth.rain_field_db(m, m, seed=3), nan=-15.0).astype(np.float32)
field64 = DeviceArray.from_host(field.astype(np.float64))
half = DeviceArray((1, m, nh), np.complex128)
out, counts = DeviceArray((1, nb), np.float64), DeviceArray((nb,), np.uint64)
lib = _lib.lib()


def rfft2():
    _lib.check(lib.psh_fft_rfft2_dev(field64.ptr, m, m, half.ptr), "psh_fft_rfft2_dev")


def binning():
    _lib.check(lib.psh_rapsd_half_dev(half.ptr, 1, m, m, out.ptr, counts.ptr), "psh_rapsd_half_dev")


rfft2()
synchronize()
floor_ms = m * nh * 16 / COPY_RATE * 1e3
report["binning_read_floor_ms"] = floor_ms
report["rfft2_ms"] = spread(timed(rfft2))
report["binning_ms"] = spread(timed(binning))
report["counts_ms"] = spread(timed(lambda: _lib.check(lib.psh_rapsd_counts_dev(m, m, 0, counts.ptr), "psh_rapsd_counts_dev")))
report["binning_over_floor"] = report["binning_ms"]["median"] / floor_ms
report["rapsd_ms"] = spread(timed(lambda: spectral.rapsd(field64, fft_method="hip")))
del half

stack = DeviceArray((k, m, m), np.float32)
for j in range(k):
    plane = DeviceArray.from_host(np.roll(field, 7 * j, axis=1) + np.float32(0.125 * (j % 5)))
    _lib.check(lib.psh_memcpy_d2d(stack.ptr + j * plane.nbytes, plane.ptr, plane.nbytes), "psh_memcpy_d2d")
synchronize()
report["table_ms"] = spread(timed(lambda: spectral.rapsd_table(stack)))
report["table_per_member_ms"] = report["table_ms"]["median"] / k
report["spectrum_member0_head"] = [float(v) for v in spectral.rapsd(stack.view(0), fft_method="hip")[:4]]
del stack

try:
    from oracle import build_ref

    build_ref.activate()
    from pysteps.utils import spectral as ref

    small = field[:1024, :1024].astype(np.float64)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref.rapsd(small, fft_method=np.fft)
        host.append(time.perf_counter() - t0)
    report["reference_1024_s"] = spread(host)
    report["reference_extrapolated_%d_s" % m] = float(np.median(host)) * (m / 1024.0) ** 2 * (nb / 512.0)
except ImportError:
    report["reference_1024_s"] = None

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "rapsd"), exist_ok=True)
    with open(os.path.join(root, "profiles", "rapsd", "rapsd_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
