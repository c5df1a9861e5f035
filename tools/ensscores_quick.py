"""Device time of ensemble skill and spread (``pysteps_amd.verification.ensscores``, csrc/ensscores.hip).

    python tools/ensscores_quick.py [side] [--members K] [--repeat N] [--warmup W] [--save]

Defaults: 4096^2, 48 resident float32 members, 3 warm-up calls, 20 timed calls.  Events on the library stream around
each call, median and range.  Three groups of figures, all on the same resident stack:

``kernel_*``   the entry points alone (launches and the download of the few numbers they return): the categorical pair
               kernel at 1 and 5 thresholds, the continuous pair kernel with the sums of RMSE (one), corr_p (three) and
               all seven, and the members' own sums; each beside its floor at the 6.29 TB/s copy rate of the MI355X -
               one read of the stack per pass of thresholds for the categorical kernel, 2 / T plane reads per pair for
               the continuous one (tile side T = 4 for one or two sums, 2 for more).
``spread_*`` / ``skill_*``  the public ``ensemble_spread`` / ``ensemble_skill`` for CSI, RMSE and corr_p, host arithmetic
               on the returned numbers included.
``loop_*``     the baseline: the loop over all pairs of this package's ``det_cat_fct`` / ``det_cont_fct`` on resident plane
               views, what a user could do before these functions existed; ``loop_kernel_*`` the same loop over the two
               entry points alone.

Prints one JSON line and, with ``--save``, writes it to profiles/ensscores/ensscores_quick_<side>.json.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pysteps_amd import _lib  # noqa: E402
from pysteps_amd.device import DeviceArray, Event, synchronize  # noqa: E402
from pysteps_amd.verification import detcatscores, detcontscores, ensscores  # noqa: E402
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
thresholds = [-5.0, 0.0, 5.0, 10.0, 15.0]  # dBR
npix, npairs = m * m, k * (k - 1) // 2
report = {"side": m, "members": k, "pairs": npairs, "thresholds": thresholds, "repeat": args.repeat, "warmup": args.warmup}


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
    return spread(times)


field = synth.rain_field_db(m, m, seed=3).astype(np.float32)
field[: m // 16, : m // 16] = np.nan
stack = DeviceArray((k, m, m), np.float32)
for j in range(k):
    plane = DeviceArray.from_host(np.roll(field, 7 * j, axis=1) + np.float32(0.125 * (j % 5)))
    _lib.check(_lib.lib().psh_memcpy_d2d(stack.ptr + j * plane.nbytes, plane.ptr, plane.nbytes), "psh_memcpy_d2d")
obs = DeviceArray.from_host(np.roll(field, (11, -5), axis=(0, 1)))
synchronize()
planes = [stack.view(j) for j in range(k)]
pairs = [(i, j) for i in range(k) for j in range(i + 1, k)]

plane_ms = npix * 4 / COPY_RATE * 1e3
stack_ms = k * plane_ms
report["stack_read_ms"] = stack_ms
masks = {"rmse": ensscores._SUM_MASK["rmse"], "corr_p": ensscores._SUM_MASK["corr_p"], "full": ensscores.FULL_MASK}
kernels = [("cat_1thr", lambda: ensscores._cat_pairs(stack, k, npix, thresholds[:1]), stack_ms),
           ("cat_5thr", lambda: ensscores._cat_pairs(stack, k, npix, thresholds), stack_ms * (1 if k <= 48 else 2)),
           ("own_sums", lambda: ensscores._own(stack, k, npix), 2 * stack_ms)]
for label, mask in masks.items():
    tile = 4 if bin(mask).count("1") <= 2 else 2
    kernels.append(("cont_" + label, lambda mask=mask: ensscores._cont_pairs(stack, k, npix, mask), npairs * 2.0 / tile * plane_ms))
for label, fn, floor in kernels:
    t = timed(fn)
    report["kernel_%s_ms" % label] = t
    report["kernel_%s_floor_ms" % label] = floor
    report["kernel_%s_over_floor" % label] = t["median"] / floor

with np.errstate(all="ignore"):
    for metric, kwargs in (("CSI", {"thr": 0.0}), ("RMSE", {}), ("corr_p", {})):
        report["spread_%s_ms" % metric] = timed(lambda: ensscores.ensemble_spread(stack, metric, **kwargs))
        report["skill_%s_ms" % metric] = timed(lambda: ensscores.ensemble_skill(stack, obs, metric, **kwargs))
        report["spread_%s" % metric] = float(ensscores.ensemble_spread(stack, metric, **kwargs))
        report["skill_%s" % metric] = float(ensscores.ensemble_skill(stack, obs, metric, **kwargs))

    def loop_cat():
        return [detcatscores.det_cat_fct(planes[i], planes[j], 0.0, ["csi"])["CSI"] for i, j in pairs]

    def loop_cont(name, key):
        return [detcontscores.det_cont_fct(planes[i], planes[j], [name])[key] for i, j in pairs]

    report["loop_CSI_ms"] = timed(loop_cat)
    report["loop_RMSE_ms"] = timed(lambda: loop_cont("rmse", "RMSE"))
    report["loop_corr_p_ms"] = timed(lambda: loop_cont("corr_p", "corr_p"))
    report["loop_kernel_cat_ms"] = timed(lambda: [detcatscores._counts(planes[i], planes[j], 1, npix, True, [0.0], [0.0]) for i, j in pairs])
    report["loop_kernel_cont_ms"] = timed(lambda: [detcontscores._sums(planes[i], planes[j], 1, npix, True, 0, 0.0, 0.0) for i, j in pairs])
    report["loop_floor_ms"] = npairs * 2 * plane_ms
    report["loop_CSI"] = float(np.mean(loop_cat()))
    report["loop_RMSE"] = float(np.mean(loop_cont("rmse", "RMSE")))

print(json.dumps(report))
if args.save:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles", "ensscores"), exist_ok=True)
    with open(os.path.join(root, "profiles", "ensscores", "ensscores_quick_%d.json" % m), "w") as fh:
        fh.write(json.dumps(report, indent=1) + "\n")
