"""Golden vectors for the DARTS motion estimate (``motion.get_method("darts_hip")``), written by the UNMODIFIED reference.

    python tools/make_golden_darts.py        (-> tests/golden/darts_reference.npz)

Runs pysteps/motion/darts.py ``DARTS`` of the reference package that ``oracle.build_ref`` prepares under oracle/_ref
on seeded synthetic frames quantised to 1/4 (stored as uint8 counts, so that the stored inputs are the exact inputs),
and stores per case: the keyword arguments, the output, the singular values of the reference's ``M^H M`` (recorded by
wrapping the module's ``svd`` / ``lstsq`` names, which pass every call through unchanged) and, for one case, the
printed text with its timings removed.  Spatial outputs larger than 64 x 80 are stored on every 4th row and column
(the field holds at most 25 Fourier bins per component; the stage tests compare whole fields).  The float32 case is
run twice: on the float32 frames (the reference's FFT then runs in complex64) and on the same values as float64.
Needs the reference; never runs on the GPU machine.
"""
import contextlib
import io
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "darts_reference.npz")
FULL_LIMIT = 64 * 80  # spatial outputs up to this many pixels are stored whole
STRIDE = 4


def q4(a):
    return np.clip(np.round(np.asarray(a, dtype=np.float64) * 4.0), 0, 255) / 4.0


def rain(m, n, T, seed):
    db = synth.steps_frames(m, n, n_frames=T, seed=seed).astype(np.float64)
    return q4(np.maximum(db + 15.0, 0.0) * 1.2)


def blob(m, n, T, width):
    yy, xx = np.mgrid[0:m, 0:n]
    return q4(np.stack([63.0 * np.exp(-((yy - m / 2 - 0.7 * t) ** 2 + (xx - n / 2 - 1.1 * t) ** 2) / (2 * width ** 2))
                        for t in range(T)]))


def noise(m, n, T, seed):
    return q4(np.random.default_rng(seed).random((T, m, n)) * 40.0)


def strip_times(text):
    text = re.sub(r"Done in [0-9.]+ seconds\.", "Done in <t> seconds.", text)
    return re.sub(r"--- [0-9.eE+-]+ seconds ---", "--- <t> seconds ---", text)


def main():
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.motion import darts

    seen = {}

    def svd_rec(a, *args, **kwargs):
        res = np.linalg.svd(a, *args, **kwargs)
        seen["s"] = np.asarray(res[1]).copy()
        return res

    def lstsq_rec(a, b, *args, **kwargs):
        MM = np.dot(a.conjugate().T, a)
        seen["s"] = np.linalg.svd(MM, compute_uv=False)
        return np.linalg.lstsq(a, b, *args, **kwargs)

    darts.svd, darts.lstsq = svd_rec, lstsq_rec

    out = {"versions": json.dumps({"numpy": np.__version__})}
    frames = {}
    cases = []

    def case(name, key, kwargs, dtype=np.float64, text=False):
        x = frames[key]
        kw = dict(kwargs)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = darts.DARTS(x.astype(dtype), **kw)
        cases.append(name)
        out[name + "__frames"] = np.array(key)
        out[name + "__dtype"] = np.array(np.dtype(dtype).name)
        out[name + "__kwargs"] = np.array(json.dumps(kw))
        out[name + "__s"] = seen.pop("s")
        if kw.get("output_type", "spatial") == "spatial" and res.shape[1] * res.shape[2] > FULL_LIMIT:
            res = res[:, ::STRIDE, ::STRIDE]
            out[name + "__stride"] = np.array(STRIDE)
        else:
            out[name + "__stride"] = np.array(1)
        out[name + "__out"] = res
        if text:
            out[name + "__text"] = np.array(strip_times(buf.getvalue()))
        return res

    def add(key, x):
        frames[key] = x
        out["frames__" + key] = (x * 4.0).astype(np.uint8)

    add("rain_128", rain(128, 128, 6, seed=11))
    add("rain_53x60", rain(53, 60, 6, seed=12))
    add("rain_64x80", rain(64, 80, 6, seed=13))
    add("rain_201x333", rain(201, 333, 9, seed=14))
    add("rain_96x128", rain(96, 128, 5, seed=15))
    add("rain_96", rain(96, 96, 6, seed=16))
    add("blob_96", blob(96, 96, 6, 6.0))
    add("noise_4x5", noise(4, 5, 6, seed=17))

    case("defaults_128", "rain_128", {"verbose": True}, text=True)
    case("min_53x60", "rain_53x60", {"verbose": False})
    case("alias_64x80", "rain_64x80", {"verbose": False})
    case("odd_201x333_T9", "rain_201x333", {"verbose": False})
    case("custom", "rain_96x128", {"N_x": 20, "N_y": 30, "N_t": 2, "M_x": 3, "M_y": 1, "verbose": False})
    case("lsq1", "rain_128", {"lsq_method": 1, "verbose": False})
    case("spectral", "rain_96", {"output_type": "spectral", "verbose": False})
    case("float32", "rain_128", {"verbose": False}, dtype=np.float32)
    case("float32_as_f64", "rain_128", {"verbose": False})
    case("cutoff", "blob_96", {"verbose": False})
    case("tiny_dup", "noise_4x5", {"N_x": 1, "N_y": 1, "N_t": 1, "verbose": False})
    out["cases"] = np.array(cases)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
