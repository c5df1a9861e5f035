"""Device time of the temporal autocorrelation (``pysteps_amd.timeseries.correlation``, csrc/autocorr.hip).

    python tools/autocorr_quick.py [side] [--levels L] [--frames T] [--repeat N] [--warmup W] [--save]

Defaults: 4096^2, 8 cascade levels, 3 frames, float64, a mask of about 35 % of the pixels, 3 warm-up calls, 20 timed
calls.  Events on the library stream around each call, median and spread.

(a) ``fused_sums``: ``psh_autocorr_sums_dev`` alone (both kernels, the result left on the device), beside
    ``floor_ms``: reading the L T planes and the mask once at the 6.29 TB/s copy rate; ``fused_over_floor`` is their
    ratio.  ``fused_sums_unmasked`` and ``fused_sums_float32`` likewise.
(b) ``public_function``: ``cascade_autocorrelation`` on the resident stack - the launch, the download of the sums and
    the rational finish on the host (host work between the events shows up as device idle time inside them).
(c) ``spectral_sums``: ``psh_autocorr_spectral_sums_dev`` on the half spectra of the same planes.
(d) ``window_one_lag``: one lag of the moving-window form (sigma 50) on two of the planes, and its finish kernel alone.
(e) ``reference_1024_s``: the unmodified reference's ``temporal_autocorrelation`` on the host at 1024^2 for the same
    L levels (L x (T - 1) coefficients), measured there; ``reference_extrapolated_<side>_s`` is that times the area
    ratio and is labelled as such.
Prints one JSON line and, with ``--save``, writes it to profiles/autocorr/autocorr_quick_<side>.json.
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
from pysteps_amd.timeseries import correlation  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("side", nargs="?", type=int, default=4096)
ap.add_argument("--levels", type=int, default=8)
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--save", action="store_true")
args = ap.parse_args()

COPY_RATE = 6.29e12  # bytes / s, the device's measured copy rate (README)
m = n = args.side
L, T = args.levels, args.frames
npix = m * n
report = {"size": m, "levels": L, "frames": T, "repeat": args.repeat, "warmup": args.warmup}


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


def planes(side, seed):
    """(L, T, side, side) float64: per level a common field plus a fresh one per frame, and a mean beside the spread."""
    rng = np.random.default_rng(seed)
    for l in range(L):
        common = rng.standard_normal((side, side))
        for t in range(T):
            yield l, t, common + 0.5 * rng.standard_normal((side, side)) + (1.0 + l)


lib = _lib.lib()
stack = DeviceArray((L, T, m, n), np.float64)
for l, t, plane in planes(m, 1):
    _lib.check(lib.psh_memcpy_h2d(stack.ptr + (l * T + t) * npix * 8, plane.ctypes.data, plane.nbytes), "h2d")
    synchronize()
mask_host = np.random.default_rng(2).random((m, n)) < 0.35
mask = DeviceArray.from_host(mask_host.view(np.uint8))
nsums = 2 + 3 * (T - 1)
out = DeviceArray((L * nsums * 2 + 1 + L,), np.float64)


def fused(x, f64, mask_ptr):
    _lib.check(lib.psh_autocorr_sums_dev(x.ptr, f64, L, T, npix, mask_ptr, 0, out.ptr, out.ptr + L * nsums * 16,
                                         out.ptr + L * nsums * 16 + 8), "psh_autocorr_sums_dev")


# (a) the fused sums
floor_ms = (L * T * npix * 8 + npix) / COPY_RATE * 1e3
report["fused_sums_ms"] = spread(timed(lambda: fused(stack, 1, mask.ptr)))
report["floor_ms"] = floor_ms
report["fused_over_floor"] = report["fused_sums_ms"]["median"] / floor_ms
report["fused_sums_unmasked_ms"] = spread(timed(lambda: fused(stack, 1, None)))
stack32 = DeviceArray((L, T, m, n), np.float32)
_lib.check(lib.psh_convert_dev(stack.ptr, stack32.ptr, stack.size, 0), "psh_convert_dev")
report["fused_sums_float32_ms"] = spread(timed(lambda: fused(stack32, 0, mask.ptr)))
report["floor_float32_ms"] = (L * T * npix * 4 + npix) / COPY_RATE * 1e3
del stack32

# (b) the public function
gamma = {}
report["public_function_ms"] = spread(timed(lambda: gamma.update(g=correlation.cascade_autocorrelation(stack, mask=mask))))
report["gamma"] = [[float(v) for v in row] for row in gamma["g"]]

# (c) the spectral sums
nc = n // 2 + 1
spectra = DeviceArray((L, T, m, nc), np.complex128)
for i in range(L * T):
    _lib.check(lib.psh_fft_rfft2_dev(stack.ptr + i * npix * 8, m, n, spectra.ptr + i * m * nc * 16), "psh_fft_rfft2_dev")
sp_sums = 1 + 2 * (T - 1)
sp_out = DeviceArray((L * sp_sums * 2 + L,), np.float64)
report["spectral_sums_ms"] = spread(timed(lambda: _lib.check(lib.psh_autocorr_spectral_sums_dev(
    spectra.ptr, L, T, m, nc, n, 0, 0, sp_out.ptr, sp_out.ptr + L * sp_sums * 16), "psh_autocorr_spectral_sums_dev")))
report["spectral_floor_ms"] = L * T * m * nc * 16 / COPY_RATE * 1e3
report["gamma_spectral"] = [[float(v) for v in row] for row in
                            correlation.cascade_autocorrelation(spectra, domain="spectral", x_shape=(m, n))]
del spectra

# (d) one moving-window lag
SIGMA = 50
pair = DeviceArray((2, m, n), np.float64)
_lib.check(lib.psh_memcpy_d2d(pair.ptr, stack.ptr, 2 * npix * 8), "d2d")
report["window_sigma"] = SIGMA
report["window_one_lag_ms"] = spread(timed(lambda: correlation.temporal_autocorrelation(pair, mask=mask, window_radius=SIGMA)))
six = DeviceArray((6, m, n), np.float64).fill_bytes(0)
cc = DeviceArray((m, n), np.float64)
p = [six.ptr + j * npix * 8 for j in range(6)]
report["window_finish_kernel_ms"] = spread(timed(lambda: _lib.check(
    lib.psh_window_corrcoef_dev(p[0], p[1], p[2], p[3], p[4], p[5], float(SIGMA**2), npix, cc.ptr), "psh_window_corrcoef_dev")))
report["window_finish_floor_ms"] = 7 * npix * 8 / COPY_RATE * 1e3
del six, cc, pair, stack

# (e) the reference on the host at 1024^2
from oracle import build_ref  # noqa: E402

build_ref.activate()
from pysteps.timeseries.correlation import temporal_autocorrelation as reference  # noqa: E402

small = np.empty((L, T, 1024, 1024))
for l, t, plane in planes(1024, 1):
    small[l, t] = plane
small_mask = np.random.default_rng(2).random((1024, 1024)) < 0.35
t0 = time.perf_counter()
ref_gamma = [reference(small[l], mask=small_mask) for l in range(L)]
report["reference_1024_s"] = time.perf_counter() - t0
report["reference_1024_label"] = "measured on this host: %d levels x %d lags" % (L, T - 1)
report["reference_extrapolated_%d_s" % m] = report["reference_1024_s"] * (m / 1024.0) ** 2
report["reference_extrapolated_label"] = "extrapolated by the area ratio, not measured"
report["reference_threads"] = os.environ.get("OMP_NUM_THREADS")

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "autocorr"), exist_ok=True)
    with open(os.path.join(root, "profiles", "autocorr", "autocorr_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
