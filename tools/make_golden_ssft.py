"""Golden vectors for the short-space Fourier (ssft / nested) noise, written by the UNMODIFIED reference.

    python tools/make_golden_ssft.py        (-> tests/golden/ssft_reference.npz, tests/golden/ssft_bars.json)

Runs pysteps/noise/fftgenerators.py ``initialize_nonparam_2d_ssft_filter``, ``initialize_nonparam_2d_nested_filter`` and
``generate_noise_2d_ssft_filter`` of the reference package that ``oracle.build_ref`` prepares under oracle/_ref on the
cases of tests/helpers/ssft.py and stores per case:

* ``field``, ``kwargs`` (JSON), ``kind`` ("ssft" / "nested");
* the reference's 4-D filter array as its distinct planes (``planes``, compared bit for bit) and the map ``plane_of``
  (``F = planes[plane_of]``) - windows that did not pass the wet-area test hold the same plane;
* ``rects`` and ``counts``: the rectangles the reference handed to ``_get_mask`` and its integers
  ``np.sum(field * mask > 0.01)``, in the order of its loops, taken by wrapping ``_get_mask`` and the first call of
  ``initialize_nonparam_2d_fft_filter`` (whose argument is the prepared stack);
* ``amp``: the factor of the filter bar (helpers/ssft.py ``filter_bar``);
* for the noise cases and seeds: ``noise_<seed>`` (``generate_noise_2d_ssft_filter(F, seed=seed)``) and ``gain_<seed>``.

The bars (``ssft_bars.json``): every case a second time in long double along the half-spectrum route
(helpers/ssft.py with helpers/fft_pointwise.py's extended-precision transform) and the REFERENCE's own deviation from
that - ``deviation_filter``: largest difference over a plane relative to the plane's largest value; ``deviation_noise``:
largest absolute difference of a noise field - each the maximum over the cases.

Needs the reference; never runs on the GPU machine.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _traced(ref, call):
    """Run ``call`` with the reference's ``_get_mask`` and inner initialiser wrapped: (result, rectangles, counts)."""
    own_mask, own_init = ref._get_mask, ref.initialize_nonparam_2d_fft_filter
    masks, prepared = [], []

    def get_mask(Size, idxi, idxj, win_fun):
        mask = own_mask(Size, idxi, idxj, win_fun)
        masks.append(((int(idxi[0]), int(idxi[1]), int(idxj[0]), int(idxj[1])), mask))
        return mask

    def init(field, **kwargs):
        if not prepared:
            prepared.append(field.copy())
        return own_init(field, **kwargs)

    ref._get_mask, ref.initialize_nonparam_2d_fft_filter = get_mask, init
    try:
        with np.errstate(divide="ignore"):
            result = call()
    finally:
        ref._get_mask, ref.initialize_nonparam_2d_fft_filter = own_mask, own_init
    rects = np.array([r for r, _ in masks], dtype=np.int64).reshape(-1, 4)
    counts = np.array([int(np.sum((prepared[0] * mask[None, :, :]) > 0.01)) for _, mask in masks], dtype=np.int64)
    return result, rects, counts


def generate():
    from helpers import ssft as hs
    from oracle import build_ref
    from pysteps_amd.noise import ssft as geo

    build_ref.build()
    build_ref.activate()
    from pysteps.noise import fftgenerators as ref

    out = {"versions": np.array(json.dumps({"numpy": np.__version__}))}
    dev = {"filter": 0.0, "noise": 0.0}
    names = []
    for kind, cases in (("ssft", hs.SSFT_CASES), ("nested", hs.NESTED_CASES)):
        for name, (shape, nr, field_kind, kw) in cases.items():
            names.append(name)
            field = hs.field(shape, nr, field_kind)
            before = field.copy()
            if kind == "ssft":
                F, rects, counts = _traced(ref, lambda: ref.initialize_nonparam_2d_ssft_filter(field, **kw))
            else:
                F, rects, counts = _traced(ref, lambda: ref.initialize_nonparam_2d_nested_filter(field, **kw))
            assert np.array_equal(field, before) and F["use_full_fft"] and tuple(F["input_shape"]) == shape
            F4 = F["field"]
            planes, plane_of = hs.dedupe(F4)
            n = shape[1]
            # the same case in long double along the half-spectrum route
            amp = []
            if kind == "ssft":
                half_ld, map_ld, counts_ld, rects_ld = hs.ssft_bank(field, np.longdouble, amp, **kw)
                assert np.array_equal(rects_ld, rects) and np.array_equal(counts_ld.ravel(), counts)
                F4_ld = geo.expand_half(half_ld, n)[map_ld]
            else:
                half_ld, counts_ld = hs.nested_bank(field, 1.0, np.longdouble, amp, **kw)
                assert np.array_equal(np.concatenate(counts_ld) if counts_ld else np.zeros(0, np.int64), counts)
                F4_ld = geo.expand_half(half_ld, n)
            dev["filter"] = max(dev["filter"], hs.plane_deviation(F4, F4_ld))
            out[hs.key(name, "kind")] = np.array(kind)
            out[hs.key(name, "field")] = field
            out[hs.key(name, "kwargs")] = np.array(json.dumps(kw))
            out[hs.key(name, "planes")] = planes
            out[hs.key(name, "plane_of")] = plane_of
            out[hs.key(name, "rects")] = rects
            out[hs.key(name, "counts")] = counts
            out[hs.key(name, "amp")] = np.array(max(amp))
            if name in hs.NOISE_CASES:
                folded = geo.fold_half(planes.astype(np.longdouble))
                for seed in hs.NOISE_SEEDS:
                    state = np.random.get_state()
                    noise = ref.generate_noise_2d_ssft_filter(F, seed=seed)
                    np.random.set_state(state)
                    white = np.random.RandomState(seed).randn(*shape)
                    det = {}
                    noise_ld = hs.generate(folded, plane_of, white, dtype=np.longdouble, details=det)
                    dev["noise"] = max(dev["noise"], hs.field_deviation(noise, noise_ld))
                    out[hs.key(name, "noise_%d" % seed)] = noise
                    out[hs.key(name, "gain_%d" % seed)] = np.array(det["gain"])
    out["cases"] = np.array(names)
    bars = {
        "deviation_filter": dev["filter"],
        "deviation_noise": dev["noise"],
        "bar_factor": hs.BAR_FACTOR,
        "unit": "filter planes: largest |difference| over a plane / the plane's largest value; noise fields: largest |difference|",
        "measured_with": {"numpy": np.__version__, "longdouble_eps": float(np.finfo(np.longdouble).eps)},
    }
    return out, bars


def main():
    from helpers import ssft as hs

    out, bars = generate()
    np.savez_compressed(hs.GOLDEN_FILE, **out)
    with open(hs.BARS_FILE, "w") as fh:
        json.dump(bars, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%s: %d cases, %d bytes" % (hs.GOLDEN_FILE, len(out["cases"]), os.path.getsize(hs.GOLDEN_FILE)))
    for name in out["cases"]:
        print("  %-10s planes %s map %s counts %s amp %.3g" % (name, out[hs.key(name, "planes")].shape, out[hs.key(name, "plane_of")].tolist(),
                                                               out[hs.key(name, "counts")].tolist(), float(out[hs.key(name, "amp")])))
    print(bars)


if __name__ == "__main__":
    main()
