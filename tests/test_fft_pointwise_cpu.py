"""The pointwise oracle of the transforms (helpers/fft_pointwise.py), checked on the CPU alone.

1. The oracle (numpy.fft in long double) against closed forms in long double, for the impulses and tones of every shape,
   the phase reduced exactly in integers: within 64 long-double eps of the output's root mean square in every bin.  Where
   the output is a single spike (the transform of a tone, the inverse of an impulse's spectrum) the spike is sqrt(m n)
   root mean squares large, and the last butterflies of ANY arithmetic add and cancel partial sums of the spike's size in
   every bin: there the bound is 64 eps of the spike's magnitude (measured: 612 eps x rms in the spike of 8192x34, 66 in
   another bin of 4096x6, where sqrt(m n) is 528 and 157).
2. tests/golden/fft_pointwise_bars.json reproduces from the case list, and the float64 restatement of the chirp-z kernel
   stays under its class's bar on every chirp case.
3. The comparator has teeth where the whole-array relative L2 of tests/test_fft_gpu.py (1e-12) has none: seeded defects.
"""

import json

import numpy as np
import pytest

from helpers import fft_pointwise as fp
from helpers import fft_pointwise_cases as pc

OLD_TOL = 1e-12  # tests/test_fft_gpu.py
_MEASURED = {}
_ALL_SHAPES = list(dict.fromkeys([s for s, _ in pc.SHAPES] + pc.FOURSTEP_SHAPES))


def _measured(shape, op):
    if (shape, op) not in _MEASURED:
        _MEASURED[(shape, op)] = pc.measure(shape, op)
    return _MEASURED[(shape, op)]


@pytest.fixture(scope="module")
def bars():
    return fp.load_bars()


def test_long_double_is_extended_precision():
    assert fp.LD_EPS < 2e-19
    assert np.fft.rfft2(np.zeros((4, 4), np.longdouble)).dtype == np.clongdouble


def _closed(got, want, note, spike=False):
    want = np.asarray(want)
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    scale = np.max(np.abs(want)) if spike else rms
    err = np.abs(got - want)
    at = np.unravel_index(int(np.argmax(err)), err.shape)
    print(note, "worst %.2f ld eps x rms at %s" % (float(err[at] / (fp.LD_EPS * rms)), at))
    assert err[at] <= 64 * fp.LD_EPS * scale, note + (at, float(err[at] / (fp.LD_EPS * scale)))


@pytest.mark.parametrize("shape", [s for s, _ in pc.SHAPES], ids=pc.shape_name)
def test_oracle_against_closed_forms(shape):
    m, n = shape
    nc = n // 2 + 1
    for at in pc.impulse_points(shape):
        x = np.zeros(shape, np.longdouble)
        x[at] = 1
        spec = fp.impulse_spectrum(shape, at)
        _closed(np.fft.fft2(x.astype(np.clongdouble)), spec, ("impulse", at, "fft2"))
        _closed(np.fft.rfft2(x), spec[:, :nc], ("impulse", at, "rfft2"))
        _closed(np.fft.ifft2(spec), x, ("impulse", at, "ifft2"), spike=True)
        _closed(np.fft.irfft2(spec[:, :nc], s=shape), x, ("impulse", at, "irfft2"), spike=True)
    for at in pc.tone_bins(shape):
        z = fp.tone(shape, at)
        spike = np.zeros(shape, np.clongdouble)
        spike[at] = m * n
        mirror = np.zeros(shape, np.clongdouble)
        mirror[(-at[0]) % m, (-at[1]) % n] = m * n
        half = (0.5 * (spike + mirror))[:, :nc]  # the spectrum of Re z
        _closed(np.fft.fft2(z), spike, ("tone", at, "fft2"), spike=True)
        _closed(np.fft.ifft2(spike), z, ("tone", at, "ifft2"))
        _closed(np.fft.rfft2(z.real), half, ("tone", at, "rfft2"), spike=True)
        _closed(np.fft.irfft2(half, s=shape), z.real, ("tone", at, "irfft2"))


@pytest.mark.parametrize("shape", _ALL_SHAPES, ids=pc.shape_name)
def test_yardsticks_and_restatement(shape, bars):
    """Measures the shape's yardsticks (kept for test_bars_file_reproduces) and holds the restatement to its class's bar
    and to the bar of its input family."""
    cls = fp.shape_class(shape)
    ops = [op for op in fp.OPS if shape in pc.shapes_of(op)]
    for op in ops:
        for fam, kinds in _measured(shape, op).items():
            for kind, (val, name) in kinds.items():
                print("%-8s %-9s %-34s %10.3f u" % (op, kind, name, val))
                assert val <= fp.bar(bars, cls, op), (op, kind, name, val)
                assert val <= fp.case_bar(bars, cls, op, fam), (op, kind, name, val)


def test_bars_file_reproduces(bars):
    """Every C of tests/golden/fft_pointwise_bars.json recomputed from the case list equals the file, the bars are 4 C."""
    got = pc.bars_from({so: _measured(*so) for so in pc.all_measurements()})
    assert json.loads(json.dumps(got)) == bars
    for cls in bars["classes"].values():
        for entry in cls.values():
            assert entry["bar"] == round(4.0 * entry["C"], 3)
            assert all(f["bar"] == round(4.0 * f["C"], 3) and f["C"] <= entry["C"] for f in entry["families"].values())


# ---- seeded defects ---------------------------------------------------------------------------------------------------
def _verdict(got, want, bar, note):
    err, at = fp.compare(got, want)
    l2 = fp.rel_l2(got, want)
    print("%-60s err %.4g u at %s (bar %.4g), whole-array rel-L2 %.3g" % (note, err, at, bar, l2))
    return err, l2


def test_one_bin_moved_by_64_units(bars):
    """64x128-noise, rfft2 of numpy in float64 with bin (40, 33) moved by 64 u: fails the case's bar (its family's),
    passes the 1e-12 whole-array bar by four orders of magnitude."""
    shape = (64, 128)
    x, want = pc.inputs(shape, "rfft2")["noise"], pc.wants(shape, "rfft2")["noise"]
    got = fp.numpy_f64("rfft2", x, shape).copy()
    bar = fp.case_bar(bars, "plain", "rfft2", "noise")
    assert _verdict(got, want, bar, "unharmed")[0] <= bar
    got[40, 33] += 64 * fp.unit(want)
    err, l2 = _verdict(got, want, bar, "one bin + 64 u")
    assert err > bar and l2 < OLD_TOL


def test_two_neighbouring_bins_swapped(bars):
    """64x128-rain, rfft2: two neighbouring bins of a row trade places.  Of all neighbouring pairs the one is taken whose
    values differ least while still differing by more than twice the case's bar - the swap a whole-array norm has the best
    chance to miss.  It fails the pointwise bar by eleven orders of magnitude.  The 1e-12 whole-array bar sees it as well
    (measured: rel-L2 1.6e-4; the least different pair of the field's spectrum is 1.2e-4 of the array norm apart), so
    unlike the defects next to it this one does not show the gap, and nothing is asserted about the old bar here."""
    shape = (64, 128)
    x, want = pc.inputs(shape, "rfft2")["rain"], pc.wants(shape, "rfft2")["rain"]
    got = fp.numpy_f64("rfft2", x, shape).copy()
    bar = fp.case_bar(bars, "plain", "rfft2", "rain")
    diff = np.abs(got[:, 1:] - got[:, :-1])
    diff[diff <= 2 * bar * fp.unit(want)] = np.inf
    r, c = np.unravel_index(int(np.argmin(diff)), diff.shape)
    got[r, c], got[r, c + 1] = got[r, c + 1], got[r, c]
    err, l2 = _verdict(got, want, bar, "bins (%d, %d) and (%d, %d) swapped" % (r, c, r, c + 1))
    assert err > bar
    print("the least different pair differs by %.3g of the array norm" % (l2 / np.sqrt(2.0)))
    assert l2 > OLD_TOL  # (the record of the sentence above)


def test_nyquist_imaginary_part_kept(bars):
    """64x128-noise, irfft2: the Nyquist column of the spectrum gets an imaginary part of 2^-40 of the spectrum's root
    mean square.  numpy's rule drops what is left of it after the column pass.  The defect keeps it the way the kernel
    would if fft_rows_c2r did not clear it: rows a and b of a pair travel as Z = A + i B, so Im A[n/2] ends up in row b
    and -Im B[n/2] in row a, each with the weight (-1)^c / n of the bin in a c2c inverse.  Fails the case's bar, passes
    1e-12."""
    shape = (64, 128)
    m, n = shape
    spec = pc.inputs(shape, "irfft2")["noise"].copy()
    rng = np.random.default_rng(3)
    spec[:, n // 2] += 1j * 2.0 ** -40 * np.sqrt(np.mean(np.abs(spec) ** 2)) * rng.standard_normal(m)
    want = fp.oracle("irfft2", spec, shape)
    bar = fp.case_bar(bars, "plain", "irfft2", "noise")
    got = fp.numpy_f64("irfft2", spec, shape)
    assert _verdict(got, want, bar, "numpy's rule")[0] <= bar
    leak = np.fft.ifft(spec, axis=0)[:, n // 2].imag[:, None] * ((-1.0) ** np.arange(n))[None, :] / n
    got = got.copy()
    got[0::2] -= leak[1::2]
    got[1::2] += leak[0::2]
    err, l2 = _verdict(got, want, bar, "Nyquist imaginary part kept")
    assert err > bar and l2 < OLD_TOL


def test_chirp_angle_without_the_modular_reduction(bars):
    """4095x6-noise, fft2: the restatement with the chirp angle formed as pi * j * j / n in float64."""
    shape = (4095, 6)
    x, want = pc.inputs(shape, "fft2")["noise"], pc.wants(shape, "fft2")["noise"]
    bar = fp.case_bar(bars, "chirp", "fft2", "noise")
    assert _verdict(fp.restated("fft2", x, shape), want, bar, "reduced in integers")[0] <= bar
    err, l2 = _verdict(fp.restated("fft2", x, shape, reduced=False), want, bar, "pi * j * j / n in float64")
    assert err > bar


def test_weights_rounded_to_float32(bars):
    """64x128, the weighted inverse with the Gaussian bank rounded to float32."""
    shape = (64, 128)
    x = pc.weighted_field(shape)
    w = pc.weight_banks(shape)["gauss"][1]
    want = pc.weighted_wants(shape)[("gauss", 1)]
    bar = fp.bar(bars, "plain", "irfft2")  # what the device's weighted inverse is held to
    assert _verdict(fp.numpy_f64("weighted", x, shape, w), want, bar, "float64 weights")[0] <= bar
    err, l2 = _verdict(fp.numpy_f64("weighted", x, shape, w.astype(np.float32).astype(np.float64)), want, bar, "float32 weights")
    assert err > bar
