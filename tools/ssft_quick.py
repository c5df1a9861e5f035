"""Device time of the short-space Fourier (ssft) noise (``pysteps_amd.noise.ssft``, csrc/ssft.hip).

    python tools/ssft_quick.py [side] [--win W] [--members K] [--repeat N] [--warmup W] [--save]

Defaults: 1024^2 with 128-pixel windows, 8 members, 3 warm-up calls, 20 timed calls.  Events on the library stream around
each call, median and range.  The field has rain on its left part only, so that some windows pass the wet-area test and
the others share the global filter.

(a) ``initialiser_ms``: ``initialize_nonparam_2d_ssft_filter(field, resident=True)`` - host preparation, upload, the
    wet-area counts, the global and the local filters (host work between the events shows up as device idle time).
(b) ``generator_ms``: one ``generate_noise_2d_ssft_filter`` call on the resident bank, the host's ``randn`` draw, the
    upload and the download included; ``generator_device_ms``: the composite alone on a resident white-noise plane.
(c) ``table_ms``: ``generate_noise_table`` for K members, their draws on the device included;
    ``table_device_ms``: the composite of K resident planes alone.
(d) ``distinct_planes``, ``windows`` and the transform floor: ``rfft2_ms`` and ``irfft2_ms`` of the same run and
    ``floor_ms = rfft2 + distinct_planes * irfft2`` per member - the (distinct planes + 1) transforms a composite cannot
    do without; ``generator_over_floor`` and ``table_over_floor`` are the device times over it (the table's over K floors).
(e) ``reference_512_s``: the reference's own initialiser and one generator call on the host at 512^2 with the same window
    size.  ``reference_extrapolated_<side>_s`` is that times (side / 512)^4 - the number of windows times the cost of a
    transform per window, both proportional to the area - and is labelled as what it is: not measured.
Prints one JSON line and, with ``--save``, writes it to profiles/ssft/ssft_quick_<side>.json.
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
from pysteps_amd.noise import ssft  # noqa: E402
from pysteps_amd.noise.randstate import DeviceRandomStates  # noqa: E402
from tools import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=1024)
ap.add_argument("--win", type=int, default=128)
ap.add_argument("--members", type=int, default=8)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m = n = args.side
K = args.members
report = {"size": m, "win_size": args.win, "members": K, "repeat": args.repeat, "warmup": args.warmup}


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


def field_of(side):
    """Rain on the left 45 % of the domain, no-rain (the field's minimum) elsewhere."""
    R = synth.rain_field_db(side, side, seed=3).astype(np.float64)
    R[:, int(0.45 * side):] = R.min()
    return R


lib = _lib.lib()
R = field_of(m)
kw = dict(win_size=(args.win, args.win))

# (a)
made = {}


def initialise():
    made["F"] = ssft.initialize_nonparam_2d_ssft_filter(R, resident=True, **kw)


report["initialiser_ms"] = spread(timed(initialise))
F = made["F"]
bank = F["field"]
report["distinct_planes"] = bank.nplanes
report["windows"] = int(bank.plane_of.size)
report["bank_bytes"] = int(bank.planes.nbytes)

# (b)
rs = np.random.RandomState(42)
report["generator_ms"] = spread(timed(lambda: ssft.generate_noise_2d_ssft_filter(F, randstate=rs)))
white1 = DeviceArray.from_host(np.random.RandomState(1).randn(1, m, n))
report["generator_device_ms"] = spread(timed(lambda: ssft._generate(bank, white1, 0.2, "tukey")))

# (c)
drs = DeviceRandomStates([np.random.RandomState(100 + k) for k in range(K)], m * n, n_draws=args.repeat + args.warmup)
try:
    report["table_ms"] = spread(timed(lambda: ssft.generate_noise_table(F, drs, K)))
    whiteK = drs.randn(m, n)
    report["table_device_ms"] = spread(timed(lambda: ssft._generate(bank, whiteK, 0.2, "tukey")))
finally:
    synchronize()
    drs.close()

# (d) the transforms of the same run
spectrum = DeviceArray((m, n // 2 + 1), np.complex128)
plane = DeviceArray((m, n), np.float64)
report["rfft2_ms"] = spread(timed(lambda: _lib.check(lib.psh_fft_rfft2_dev(white1.ptr, m, n, spectrum.ptr), "rfft2")))
report["irfft2_ms"] = spread(timed(lambda: _lib.check(lib.psh_fft_irfft2_dev(spectrum.ptr, m, n, plane.ptr), "irfft2")))
floor = report["rfft2_ms"]["median"] + bank.nplanes * report["irfft2_ms"]["median"]
report["floor_ms"] = floor
report["generator_over_floor"] = report["generator_device_ms"]["median"] / floor
report["table_over_floor"] = report["table_device_ms"]["median"] / (K * floor)
report["transform_share_of_generator"] = min(1.0, floor / report["generator_device_ms"]["median"])

# (e) the reference on the host at 512^2
from oracle import build_ref  # noqa: E402

build_ref.activate()
from pysteps.noise import fftgenerators as reference  # noqa: E402

small = field_of(512)
t0 = time.perf_counter()
F_ref = reference.initialize_nonparam_2d_ssft_filter(small, **kw)
t1 = time.perf_counter()
reference.generate_noise_2d_ssft_filter(F_ref, randstate=np.random.RandomState(42))
t2 = time.perf_counter()
host = {"initialiser": t1 - t0, "generator": t2 - t1}
report["reference_512_s"] = host
report["reference_extrapolated_%d_s" % m] = {k: v * (m / 512.0) ** 4 for k, v in host.items()}
report["reference_threads"] = os.environ.get("OMP_NUM_THREADS")

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "ssft"), exist_ok=True)
    with open(os.path.join(root, "profiles", "ssft", "ssft_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
