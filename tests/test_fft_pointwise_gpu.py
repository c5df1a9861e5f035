"""Every bin of the HIP transforms (csrc/fft.hip, through cascade.hip for the weighted inverse) against numpy.fft in long
double (helpers/fft_pointwise.py).

tests/test_fft_gpu.py and tests/test_cascade_gpu.py hold the transforms by a whole-array relative L2 against numpy in the
same precision, which does not see an error confined to a few bins: a chirp or twiddle table entry off in its last
digits, a DC / Nyquist bin whose imaginary part is kept, a weight applied in the wrong precision at one row.  Here every
bin is held to ``err <= bar``, err in u = 2^-53 x the root mean square of the oracle's output, the bars 4 x the largest
value the CPU yardsticks show (tests/golden/fft_pointwise_bars.json, reproduced by tests/test_fft_pointwise_cpu.py): per
class ("plain": both sides powers of two, "chirp": not) and operation as the case list's worst, and per input family,
since the class's worst is set by the families whose output holds one spike sqrt(m n) root mean squares large.

Which case pins which branch of fft.hip (helpers/fft_pointwise_cases.py::SHAPES carries the same per shape):
  fft_lds, first radix-2 layer of an odd logn          2x2, 4x8 (n), 8x32, 64x128 (n), 2x8192, 3x8192
  fft_lds, 0 / 1 / 2 / 3 fft_pass16 rounds             2x2, 4x8 / 16x2, 8x32, 64x128 / 256x16, 512x*, 1024x*, 2048x*, 4096x* / *x8192
  fft_lds, the final pair of layers                    4x8, 64x128, 1024x6, 2048x6
  fft_cols_c2c, two columns per workgroup              512x6, 4096x6, and every column length below 1024
  fft_cols_c2c, narrow form                            1024x6, 2048x6, 1024x34
  fft_cols_c2c, c < live with one live column          512x4, 128x12 (rfft2 / irfft2: nc = 3, 7), 17x31, 2047x3 (c2c)
  fft_cols_c2c, g >= groups                            2x2, 512x2, 128x34, 1024x34 (groups 1, 1, 9 / 17, 18 / 34)
  fft_rows_r2c / c2r, rb = min(ra + 1, m - 1)          3x8, 127x16, 4095x2, 3x8192, 3x5, 7x2, 17x31, 1023x2, ...
  rows at the LDS limit                                2x8192, 3x8192
  fft_cols_step, default path                          8192x2, 8192x6 (chirp rows, nc = 4 < one tile), 8192x34 (partial tile)
  fft_cols_step at 1024 / 2048 / 4096 points           helpers/fft_fourstep_child.py (PYSTEPS_HIP_FFT_FOURSTEP=2)
  dft_pre / dft_lds / dft_out, chirp-z                 3x5, 7x2, 2x7, 17x31, 1023x2, 1025x2, 2047x3, 2049x3, 4095x6, 6x4095,
                                                       100x64, 64x100, 640x710
  fft_rows_c2r, bin 0 / Nyquist imaginary parts        the "nonhermitian" spectra of every shape (even and odd n)
  weights != nullptr in both column kernels            test_weighted_inverse: 64x128, 100x64, 1024x6 / 8192x6, 8192x34

The bars were set before any device run and rest on the CPU measurement alone.  Where the device misses one, that is a
finding about the kernel or about the restatement, to be explained in DESIGN.md next to the FFT section with the failing
input kept as a named case - not a reason to widen a bar.  What was seen is appended to fft_pointwise_seen.jsonl in the
directory named by PYSTEPS_HIP_SEEN_DIR, when that is set.

Seen on an MI355X (worst err in u / bar): dense families (noise, non-Hermitian spectra) plain rfft2 11.0 / 38.0, irfft2
11.0 / 42.7, fft2 8.5 / 40.4, ifft2 9.0 / 38.4; chirp rfft2 17.6 / 69.4, irfft2 29.3 / 92.6, fft2 20.8 / 79.9, ifft2
20.4 / 87.1; weighted inverse plain 13.6 / 64.7, chirp 29.3 / 130.4.  All families against the class bar: plain rfft2
59.1 / 209.4, irfft2 130.6 / 271.6, fft2 107.0 / 427.9, ifft2 139.7 / 278.7; chirp rfft2 1107 / 4429, irfft2 1358 / 5431,
fft2 2349 / 6254, ifft2 1420 / 5779.

What the first device run found: with W_2h^j formed in flight as the square of W_4h^j (radix4 of fft.hip) two cases missed
their bar in the one spike bin of the output - 64x128 rfft2 of tone@1,1, bin (1, 1): 250.4 u against 170.9 (family) and
209.4 (class); 640x710 fft2 of mean1e6, bin (0, 0): 3037 u against 2536 - and the dense families stood at 13 - 17 u
(plain) and 31 - 47 u (chirp).  A float64 restatement of the kernel's butterflies gave the same 250.4 u on the CPU and
28.4 u with W_2h^j read from the table; the kernel reads it from the table since, and both inputs stay named cases
(64x128-tone@1,1, 640x710-mean1e6).
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import fft_pointwise as fp
from helpers import fft_pointwise_cases as pc

pytestmark = pytest.mark.gpu

TRANSFORMS = fp.OPS[:4]
_SHAPES = list(dict.fromkeys([s for s, _ in pc.SHAPES] + pc.FOURSTEP_SHAPES))  # the child's shapes in one sweep as well
PATTERN = 0xA5


def _seen(rec):
    out_dir = os.environ.get("PYSTEPS_HIP_SEEN_DIR")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        rec = dict(rec, test=os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0])
        with open(os.path.join(out_dir, "fft_pointwise_seen.jsonl"), "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def bars():
    return fp.load_bars()


def _lib():
    from pysteps_amd import _lib

    return _lib


def _dev(a):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(a))


def _empty(shape, dtype):
    from pysteps_amd.device import DeviceArray

    return DeviceArray(shape, dtype)


def _host(d):
    return np.array(d.to_host(), copy=True)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype in (np.float64, np.complex128) else a


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _out_spec(op, shape):
    m, n = shape
    return {"rfft2": ((m, n // 2 + 1), np.complex128), "irfft2": ((m, n), np.float64), "fft2": ((m, n), np.complex128),
            "ifft2": ((m, n), np.complex128)}[op]


# ---- 1. the four transforms, every bin --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,op", [(s, op) for s in _SHAPES for op in TRANSFORMS],
                         ids=lambda v: pc.shape_name(v) if isinstance(v, tuple) else v)
def test_every_bin(shape, op, bars):
    cls = fp.shape_class(shape)
    want = pc.wants(shape, op)
    worst = {}
    for key, x in pc.inputs(shape, op).items():
        before = x.copy()
        got = fp.device_op(op, x, shape)
        oshape, odtype = _out_spec(op, shape)
        assert got.shape == oshape and got.dtype == odtype
        err, at = fp.compare(got, want[key])
        fam = pc.family(key)
        bar = fp.case_bar(bars, cls, op, fam)
        print("%-8s %-28s %10.3f u at %-12s bar %.3f" % (op, pc.shape_name(shape) + "-" + key, err, at, bar))
        worst[fam] = max(worst.get(fam, 0.0), err)
        _seen(dict(shape=list(shape), cls=cls, op=op, case=key, family=fam, err=err, at=list(at), bar=bar))
        assert err <= bar, (pc.shape_name(shape), op, key, "worst bin", at, err, "bar", bar)
        assert np.array_equal(before, x)
        if key == "noise":  # once per shape: DeviceArray in -> DeviceArray out, the same bytes, the input untouched
            d_x = _dev(x)
            d_got = fp.device_op(op, d_x, shape)
            assert _same_bits(_host(d_got), np.ascontiguousarray(got)), (shape, op, "DeviceArray route differs")
            assert _same_bits(_host(d_x), np.ascontiguousarray(x)), (shape, op, "input written")


# ---- 2. the weighted inverse ------------------------------------------------------------------------------------------
def _weighted_bar(bars, cls):
    """the irfft2 bar of the class and, being smaller, the bar of the weighted chain's own yardstick"""
    return min(fp.bar(bars, cls, "irfft2"), fp.bar(bars, cls, "weighted"))


@pytest.mark.parametrize("shape", pc.WEIGHTED_SHAPES, ids=pc.shape_name)
def test_weighted_inverse(shape, bars):
    """psh_cascade_decompose_levels_dev = irfft2(rfft2(field) x weights) per level, weights != nullptr in fft_cols_c2c
    (64x128, 100x64, 1024x6) and fft_cols_step (8192x6, 8192x34): every pixel within the irfft2 bar of the class; the
    field and a spectrum of it taken before the call are bit for bit what they were."""
    cls = fp.shape_class(shape)
    bar = _weighted_bar(bars, cls)
    field = pc.weighted_field(shape)
    d_field = _dev(field)
    d_spec = fp.device_op("rfft2", d_field, shape)
    spec_before = _host(d_spec)
    want = pc.weighted_wants(shape)
    for name, bank in pc.weight_banks(shape).items():
        got = fp.device_weighted(d_field, bank, shape)
        for k in range(pc.N_LEVELS):
            err, at = fp.compare(got[k], want[(name, k)])
            print("weighted %-22s %10.3f u at %-12s bar %.3f" % ("%s-%s[%d]" % (pc.shape_name(shape), name, k), err, at, bar))
            _seen(dict(shape=list(shape), cls=cls, op="weighted", case="%s[%d]" % (name, k), family=name, err=err, at=list(at),
                       bar=bar))
            assert err <= bar, (pc.shape_name(shape), name, k, "worst pixel", at, err, "bar", bar)
    assert _same_bits(_host(d_spec), spec_before)
    assert _same_bits(_host(d_field), np.ascontiguousarray(field))
    assert _same_bits(_host(fp.device_op("rfft2", d_field, shape)), spec_before)


# ---- 3. psh_fft_irfft2_min_dev ----------------------------------------------------------------------------------------
def _decode_key(key):
    key = int(key)
    bits = key & ~(1 << 63) if key >> 63 else ~key & ((1 << 64) - 1)
    return np.array([bits], np.uint64).view(np.float64)[0]


@pytest.mark.parametrize("shape", [(127, 16), (8192, 6), (3, 8192)], ids=pc.shape_name)
def test_irfft2_min(shape):
    """The field bit for bit psh_fft_irfft2_dev's, the key exactly np.min of it."""
    lib = _lib().lib()
    m, n = shape
    for key_name in ("noise", "rain", "nonhermitian"):
        d_spec = _dev(pc.inputs(shape, "irfft2")[key_name])
        field, plain = _empty((m, n), np.float64), _empty((m, n), np.float64)
        key = _dev(np.zeros(1, np.uint64))
        _lib().check(lib.psh_fft_irfft2_min_dev(d_spec.ptr, m, n, field.ptr, key.ptr), "psh_fft_irfft2_min_dev")
        _lib().check(lib.psh_fft_irfft2_dev(d_spec.ptr, m, n, plain.ptr), "psh_fft_irfft2_dev")
        got = _host(field)
        assert _same_bits(got, _host(plain)), (shape, key_name)
        assert _same_bits(np.array([_decode_key(_host(key)[0])]), np.array([np.min(got)])), (shape, key_name)


# ---- 4. in place ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 32), (17, 31), (1024, 6), (8192, 6)], ids=pc.shape_name)
def test_c2c_in_place(shape):
    """include/pysteps_hip.h: psh_fft_c2c2_dev takes in_dev == out_dev.  Same bytes as out of place, both directions."""
    lib = _lib().lib()
    m, n = shape
    for inverse, op in ((0, "fft2"), (1, "ifft2")):
        x = pc.inputs(shape, op)["noise"]
        d_in, d_out = _dev(x), _empty((m, n), np.complex128)
        _lib().check(lib.psh_fft_c2c2_dev(d_in.ptr, m, n, inverse, d_out.ptr), "psh_fft_c2c2_dev")
        buf = _dev(x)
        _lib().check(lib.psh_fft_c2c2_dev(buf.ptr, m, n, inverse, buf.ptr), "psh_fft_c2c2_dev")
        assert _same_bits(_host(buf), _host(d_out)), (shape, op)
        assert _same_bits(_host(d_in), np.ascontiguousarray(x))


# ---- 5. a transform writes its output and nothing else ----------------------------------------------------------------
def _framed(shape, dtype):
    """An output view inside a larger allocation: at least one output row of a fixed byte pattern before and after it,
    the view 16-byte aligned.  -> (base, view, margin in bytes)"""
    from pysteps_amd.device import DeviceArray

    dtype = np.dtype(dtype)
    row = int(shape[-1]) * dtype.itemsize
    margin = (row + 15) // 16 * 16
    nbytes = int(np.prod(shape)) * dtype.itemsize
    base = DeviceArray((2 * margin + nbytes,), np.uint8).fill_bytes(PATTERN)
    assert base.ptr % 16 == 0
    return base, DeviceArray(shape, dtype, ptr=base.ptr + margin, owner=base), margin


def _check_frame(base, margin, want, note):
    raw = _host(base)
    assert np.all(raw[:margin] == PATTERN), note + ("the bytes before the output were written",)
    assert np.all(raw[raw.size - margin:] == PATTERN), note + ("the bytes after the output were written",)
    want = np.ascontiguousarray(want)
    assert np.array_equal(raw[margin: raw.size - margin], want.view(np.uint8).ravel()), note + ("output differs",)


@pytest.mark.parametrize("shape", [(3, 8), (127, 16), (17, 31), (8192, 6), (1024, 34)], ids=pc.shape_name)
def test_writes_only_its_output(shape):
    """The odd-m row pair (rb = min(ra + 1, m - 1)), c < live in both column kernels and g >= groups: the output sits
    between two margins of a byte pattern, which come back untouched; the inputs come back untouched too."""
    lib = _lib().lib()
    m, n = shape
    calls = {
        "rfft2": lambda i, o: lib.psh_fft_rfft2_dev(i.ptr, m, n, o.ptr),
        "irfft2": lambda i, o: lib.psh_fft_irfft2_dev(i.ptr, m, n, o.ptr),
        "fft2": lambda i, o: lib.psh_fft_c2c2_dev(i.ptr, m, n, 0, o.ptr),
        "ifft2": lambda i, o: lib.psh_fft_c2c2_dev(i.ptr, m, n, 1, o.ptr),
    }
    for op in TRANSFORMS:
        x = np.ascontiguousarray(pc.inputs(shape, op)["noise"])
        d_in = _dev(x)
        oshape, odtype = _out_spec(op, shape)
        plain = _empty(oshape, odtype)
        _lib().check(calls[op](d_in, plain), op)
        base, view, margin = _framed(oshape, odtype)
        _lib().check(calls[op](d_in, view), op)
        _check_frame(base, margin, _host(plain), (shape, op))
        assert _same_bits(_host(d_in), x), (shape, op, "input written")
    # the weighted inverse: three levels in a row between the margins
    field = pc.weighted_field(shape)
    bank = pc.weight_banks(shape)["gauss"]
    d_field = _dev(field)
    want = fp.device_weighted(d_field, bank, shape)
    base, view, margin = _framed((pc.N_LEVELS, m, n), np.float64)
    fp.device_weighted(d_field, bank, shape, levels_out=view)
    _check_frame(base, margin, want, (shape, "weighted"))
    assert _same_bits(_host(d_field), np.ascontiguousarray(field))


# ---- 6. the four-step column pass at 1024 / 2048 / 4096 points --------------------------------------------------------
def test_fourstep_at_shorter_columns(bars):
    """helpers/fft_fourstep_child.py in a fresh process with PYSTEPS_HIP_FFT_FOURSTEP=2 (the switch is read once per
    process): exit status 0, a line for every case, every line within the bar of its class and family - the bars the
    same shapes are held to in one sweep by test_every_bin / the same banks by the weighted bar, so the two column passes
    stand within 4 C of each other through the oracle."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "fft_fourstep_child.py")
    done = subprocess.run([sys.executable, child], env={**os.environ, "PYSTEPS_HIP_FFT_FOURSTEP": "2"}, timeout=240,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    # (a child that died on a signal or ran out of time ends the test here: nothing is started after it)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    lines = [json.loads(l) for l in done.stdout.splitlines() if l.startswith("{")]
    expect = 0
    for shape in pc.FOURSTEP_SHAPES:
        expect += sum(len(pc.inputs(shape, op)) for op in TRANSFORMS) + 3 * pc.N_LEVELS
    assert len(lines) == expect, (len(lines), expect)
    assert {tuple(l["shape"]) for l in lines} == set(pc.FOURSTEP_SHAPES)
    for l in lines:
        cls = fp.shape_class(l["shape"])
        bar = _weighted_bar(bars, cls) if l["op"] == "weighted" else fp.case_bar(bars, cls, l["op"], l["family"])
        _seen(dict(l, cls=cls, bar=bar, fourstep=2))
        assert l["err"] <= bar, (l, "bar", bar)
