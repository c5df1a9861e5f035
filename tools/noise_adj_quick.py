"""Device time of the noise standard-deviation adjustment (``pysteps_amd.noise.utils``, csrc/noise_adj.hip).

    python tools/noise_adj_quick.py [side] [--levels L] [--iter K] [--repeat N] [--warmup W] [--save]

Defaults: 4096^2, 8 cascade levels, 20 realisations, 3 warm-up calls, 20 timed calls.  Events on the library stream
around each call, median and spread.

(a) ``whole_call_conditional`` / ``whole_call_unconditional``: ``compute_noise_stddev_adjs`` on a resident field, seed
    chain and the hand-over of the generator states included (host work between the events shows up as device idle time
    inside them).
(b) ``stages``: the pieces of one realisation - ``draw`` (all K white-noise fields in one launch, per call),
    ``filter`` (psh_noise_filter_dev), ``prepare`` (one field), ``prepare_L_fields`` (a batch of L fields: the unmasked
    moments of L whole planes - the reduction the cascade's level statistics and the noise filter share - plus the
    element-wise pass, 8 + 16 bytes per pixel and plane), ``decompose_levels`` (L inverse transforms),
    ``masked_moments_ppb1`` / ``masked_moments_ppb4`` (L planes, one / four planes per block: the measurement behind
    ``PLANES_PER_BLOCK``), ``rfft2`` and ``spectrum_moments`` (the unconditional route), ``mask_count``.
(c) ``reference_1024_s``: the reference's own function on the host at 1024^2 with the same levels and realisations, one
    call per value of ``conditional``; ``reference_extrapolated_<side>_s`` is that times the area ratio and is labelled
    as such.
Prints one JSON line and, with ``--save``, writes it to profiles/noise_adj/noise_adj_quick_<side>.json.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pysteps_amd import _lib  # noqa: E402
from pysteps_amd.cascade.decomposition import _device_weights  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from pysteps_amd.noise import utils as adj  # noqa: E402
from pysteps_amd.noise.randstate import DeviceRandomStates  # noqa: E402
from tools import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=4096)
ap.add_argument("--levels", type=int, default=8)
ap.add_argument("--iter", type=int, default=20)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

m = n = args.side
L, K = args.levels, args.iter
report = {"size": m, "levels": L, "realisations": K, "repeat": args.repeat, "warmup": args.warmup}

from oracle import build_ref  # noqa: E402

build_ref.activate()
from pysteps.cascade.bandpass_filters import filter_gaussian  # noqa: E402
from pysteps.cascade.decomposition import decomposition_fft  # noqa: E402
from pysteps.noise.fftgenerators import generate_noise_2d_fft_filter, initialize_nonparam_2d_fft_filter  # noqa: E402
from pysteps.noise.utils import compute_noise_stddev_adjs as reference  # noqa: E402


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


def inputs(side):
    R = synth.rain_field_db(side, side, seed=3).astype(np.float64)
    return R, filter_gaussian((side, side), L), initialize_nonparam_2d_fft_filter(R)


THR1, THR2 = -10.0, -15.0
R, F, noise_filter = inputs(m)
d_R = DeviceArray.from_host(R)
lib = _lib.lib()

# (a) the whole call
coeffs = {}
for conditional in (True, False):
    def call(conditional=conditional):
        coeffs[conditional] = adj.compute_noise_stddev_adjs(d_R, THR1, THR2, F, decomposition_fft, noise_filter,
                                                            generate_noise_2d_fft_filter, K, conditional=conditional, seed=42)
    label = "whole_call_conditional" if conditional else "whole_call_unconditional"
    report[label + "_ms"] = spread(timed(call))
    report[label + "_coeffs"] = [float(v) for v in coeffs[conditional]]

# (b) the stages of one realisation
plane = m * n
weights = _device_weights(F["weights_2d"])
d_filter = _device_weights(noise_filter["field"])
mask = DeviceArray((m, n), np.uint8)
clean = DeviceArray((m, n), np.float64)
_lib.check(lib.psh_noise_adj_observed_dev(d_R.ptr, plane, THR1, THR2, mask.ptr, clean.ptr), "observed")
count = adj.mask_count(mask)
white = DeviceArray((K, m, n), np.float64)
field = DeviceArray((1, m, n), np.float64)
levels = DeviceArray((L, m, n), np.float64)
spectrum = DeviceArray((m, n // 2 + 1), np.complex128)
stages = {}


def draw():
    drs = DeviceRandomStates(adj._seed_chain(42, K), plane, n_draws=1)
    drs.randn(m, n, out=white)
    synchronize()
    drs.close()


stages["seed_chain_handover_and_draw_%d_fields_ms" % K] = spread(timed(draw))
stages["filter_ms"] = spread(timed(lambda: _lib.check(lib.psh_noise_filter_dev(white.view(0).ptr, d_filter.ptr, m, n, field.ptr), "filter")))
stages["prepare_ms"] = spread(timed(lambda: adj.prepare(field, mask, 1.0, 0.0, THR2)))  # sigma 1, mu 0: the field keeps its scale
batch = DeviceArray((L, m, n), np.float64)
for k in range(L):
    _lib.check(lib.psh_noise_filter_dev(white.view(k % K).ptr, d_filter.ptr, m, n, batch.view(k).ptr), "filter")
stages["prepare_L_fields_ms"] = spread(timed(lambda: adj.prepare(batch, mask, 1.0, 0.0, THR2)))
del batch
stages["decompose_levels_ms"] = spread(timed(lambda: _lib.check(
    lib.psh_cascade_decompose_levels_dev(field.ptr, weights.ptr, L, m, n, levels.ptr), "levels")))
for ppb in (1, 4):
    stages["masked_moments_ppb%d_ms" % ppb] = spread(timed(lambda ppb=ppb: adj.masked_moments(levels, mask, count, planes_per_block=ppb)))
stages["mask_count_ms"] = spread(timed(lambda: adj.mask_count(mask)))
stages["rfft2_ms"] = spread(timed(lambda: _lib.check(lib.psh_fft_rfft2_dev(field.ptr, m, n, spectrum.ptr), "rfft2")))
stages["spectrum_moments_ms"] = spread(timed(lambda: adj.spectrum_level_moments(spectrum, weights, (m, n))))
stages["masked_moments_bytes"] = L * plane * 8 + plane
stages["spectrum_moments_bytes"] = (L * 8 + 16) * m * (n // 2 + 1)
report["stages"] = stages
del white, levels, field, spectrum, clean

# (c) the reference on the host at 1024^2, one call per value of conditional
small = inputs(1024) if m != 1024 else (R, F, noise_filter)
host = {}
for conditional in (True, False):
    t0 = time.perf_counter()
    reference(small[0], THR1, THR2, small[1], decomposition_fft, small[2], generate_noise_2d_fft_filter, K, conditional=conditional,
              seed=42)
    host["conditional" if conditional else "unconditional"] = time.perf_counter() - t0
report["reference_1024_s"] = host
report["reference_extrapolated_%d_s" % m] = {k: v * (m / 1024.0) ** 2 for k, v in host.items()}
report["reference_threads"] = os.environ.get("OMP_NUM_THREADS")

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "noise_adj"), exist_ok=True)
    with open(os.path.join(root, "profiles", "noise_adj", "noise_adj_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
