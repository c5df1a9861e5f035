"""Golden vectors for the Proesmans motion estimate (``motion.get_method("proesmans_hip")``), written by the UNMODIFIED
reference.

    python tools/make_golden_proesmans.py    (-> tests/golden/proesmans_reference.npz, proesmans_bars.json)

Runs pysteps/motion/proesmans.py ``proesmans(..., full_output=True)`` of the reference package that ``oracle.build_ref``
prepares under oracle/_ref, and the restatement of tests/helpers/proesmans.py twice: with the reference's sequential
``c_sum`` (asserted equal to the reference bit for bit) and with the exactly rounded one (what the device computes).
The frames follow one seeded recipe (helpers.proesmans.recipe_frames).  Per case the file holds

* ``<case>__kwargs`` (JSON: m, n, seed, dtype, lam, num_iter, num_levels) and ``<case>__stride``;
* ``<case>__frames`` for the two small host-only cases, whole; for the device cases the SHA-256 of the frames'
  bytes as ``<case>__frames_sha256`` - float64 noise does not compress and the whole frames of one case would fill the
  file, so the tests rebuild them from the recipe and hold them to the digest;
* ``<case>__ref_V`` (2, 2, ., .) and ``<case>__ref_G`` (2, ., .): the reference's advfield and quality on every
  ``stride``-th row and column (whole for the small cases);
* ``<case>__exact_dV``, ``<case>__exact_dG``: exact-mode restatement minus reference on the same pixels.  The tool
  asserts that reference + difference gives the restatement's bits back, so nothing is lost.

proesmans_bars.json holds each case's OWN DEVIATION: the largest difference between the reference and the exact-mode
restatement over the whole planes, for V and for GAMMA.  The algorithm amplifies the rounding of ``c_sum``, on some
inputs strongly; a device case whose own deviation exceeds 1e-8 is refused here and has to be replaced by another.
Needs the reference; never runs on the GPU machine.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import proesmans as hp  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "proesmans_reference.npz")
BARS = os.path.join(ROOT, "tests", "golden", "proesmans_bars.json")
OWN_DEVIATION_CAP = 1e-8
STORED_PIXELS = 1100  # per plane

# name, m, n, num_levels, num_iter, dtype, on the device, seed.  Seed 7 amplifies the rounding of c_sum to 1e-3 at the
# default keywords on 200 x 260 (as do 4, 6 and 9; 1, 2, 3, 5 and 8 stay below 4e-11), so that case has another one
CASES = (
    ("cpu_41x37_l2_i4", 41, 37, 2, 4, "float64", False, 7),
    ("cpu_70x33_l3_i3", 70, 33, 3, 3, "float64", False, 7),
    ("d150x131_l3_i10", 150, 131, 3, 10, "float64", True, 7),
    ("d150x131_l3_i100", 150, 131, 3, 100, "float64", True, 7),
    ("d257x193_l4_i10", 257, 193, 4, 10, "float64", True, 7),
    ("d384x320_l6_i5", 384, 320, 6, 5, "float64", True, 7),
    ("d384x320_l6_i20", 384, 320, 6, 20, "float64", True, 7),
    ("d200x260_defaults", 200, 260, 6, 100, "float64", True, 3),
    ("d150x131_l3_i10_f32", 150, 131, 3, 10, "float32", True, 7),
)


def stride_for(m, n):
    s = 1
    while -(-m // s) * -(-n // s) > STORED_PIXELS:
        s += 2
    return s


def digest(frames):
    return hashlib.sha256(np.ascontiguousarray(frames).tobytes()).hexdigest()


def case_frames(m, n, seed, dtype):
    """The frames of a case in its dtype (float32: the recipe's values rounded once)."""
    return hp.recipe_frames(m, n, seed).astype(dtype)


def main():
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.motion.proesmans import proesmans as reference

    out = {"versions": np.array(json.dumps({"numpy": np.__version__}))}
    bars = {}
    names = []
    for name, m, n, levels, iters, dtype, device, seed in CASES:
        frames = case_frames(m, n, seed, dtype)
        kw = dict(lam=50.0, num_iter=iters, num_levels=levels)
        wide = frames.astype(np.float64)  # the reference's typed memoryview takes float64 only
        ref_V, ref_G = reference(wide.copy(), full_output=True, **kw)
        seq_V, seq_G = hp.proesmans(wide, full_output=True, c_sum="sequential", **kw)
        assert np.array_equal(seq_V, ref_V) and np.array_equal(seq_G, ref_G), "%s: the restatement left the reference" % name
        ex_V, ex_G = hp.proesmans(wide, full_output=True, c_sum="exact", **kw)
        dev_V, dev_G = float(np.max(np.abs(ex_V - ref_V))), float(np.max(np.abs(ex_G - ref_G)))
        if device:
            assert dev_V <= OWN_DEVIATION_CAP and dev_G <= OWN_DEVIATION_CAP, (name, dev_V, dev_G)
        s = 1 if not device else stride_for(m, n)
        rV, rG = ref_V[..., ::s, ::s], ref_G[..., ::s, ::s]
        dV, dG = ex_V[..., ::s, ::s] - rV, ex_G[..., ::s, ::s] - rG
        assert np.array_equal(rV + dV, ex_V[..., ::s, ::s]) and np.array_equal(rG + dG, ex_G[..., ::s, ::s]), name
        names.append(name)
        out[name + "__kwargs"] = np.array(json.dumps(dict(kw, m=m, n=n, seed=seed, dtype=dtype, device=device)))
        out[name + "__stride"] = np.array(s)
        if device:
            out[name + "__frames_sha256"] = np.array(digest(frames))
        else:
            out[name + "__frames"] = frames
        out[name + "__ref_V"], out[name + "__ref_G"] = rV, rG
        out[name + "__exact_dV"], out[name + "__exact_dG"] = dV, dG
        bars[name] = {"V": dev_V, "GAMMA": dev_G}
        print("%-22s stride %2d  own deviation V %.2e GAMMA %.2e  max |V| %.2f" % (name, s, dev_V, dev_G, np.max(np.abs(ref_V))),
              flush=True)
    out["cases"] = np.array(names)
    np.savez_compressed(OUT, **out)
    with open(BARS, "w") as f:
        json.dump({"own_deviation": bars, "cap": OWN_DEVIATION_CAP}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d cases, %d bytes" % (OUT, len(names), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
