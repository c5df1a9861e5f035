"""Every bin of a two-dimensional transform against an extended-precision oracle (tests/test_fft_pointwise_*.py).

* ORACLE: ``numpy.fft`` on ``np.longdouble`` / ``np.clongdouble`` input.  numpy >= 2.0 computes these in the input's
  precision (80-bit on x86-64: eps 1.08e-19, ``rfft2`` returns complex256), with numpy's own rule for ``irfft2``: the
  imaginary parts of bin 0 and, for even lengths, of the Nyquist bin of the last axis are dropped.
* UNIT: ``u = 2^-53 sqrt(mean |oracle output|^2)`` over the whole output - what a transform's per-bin rounding error
  scales with, in both directions.
* COMPARATOR: ``max |got - oracle| / u`` over all bins and the index of the worst bin.  Not a norm.
* YARDSTICKS, measured on the CPU only: ``numpy.fft`` in float64 and, for sides that are not powers of two, a float64
  restatement of the kernel's chirp-z algorithm (``restated``): pre-multiply by ``conj(b_j)``,
  ``b_j = exp(i pi (j^2 mod 2n) / n)`` formed in long double and rounded once as csrc/fft.hip ``make_dft`` does, zero-pad
  to ``M = 2^ceil(log2(2n-1))``, ``fft``, multiply by the spectrum of the symmetric extension of ``b``, ``ifft``,
  post-multiply.  Power-of-two axes of the restatement are ``numpy.fft`` in float64.

The five operations: ``rfft2``, ``irfft2``, ``fft2``, ``ifft2`` and ``weighted`` = ``irfft2(rfft2(field) * weights)``,
the cascade's level transform (its input is the pair (field, weights)).
"""

import json
import os

import numpy as np

OPS = ("rfft2", "irfft2", "fft2", "ifft2", "weighted")
BAR_FACTOR = 4.0
LD_EPS = float(np.finfo(np.longdouble).eps)
BARS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "fft_pointwise_bars.json")


def is_pow2(v):
    return v >= 2 and (v & (v - 1)) == 0


def shape_class(shape):
    """"plain": both sides powers of two; "chirp": at least one side goes through the chirp-z transform."""
    return "plain" if all(is_pow2(int(s)) for s in shape) else "chirp"


def _ld(x):
    x = np.asarray(x)
    return x.astype(np.clongdouble if np.iscomplexobj(x) else np.longdouble)


def oracle(op, x, shape, weights=None):
    """The operation in long double.  ``x``: the float64 / complex128 input the device gets (the field for "weighted")."""
    shape = tuple(int(s) for s in shape)
    if op == "rfft2":
        return np.fft.rfft2(_ld(x))
    if op == "irfft2":
        return np.fft.irfft2(_ld(x), s=shape)
    if op == "fft2":
        return np.fft.fft2(_ld(x))
    if op == "ifft2":
        return np.fft.ifft2(_ld(x))
    if op == "weighted":
        return np.fft.irfft2(np.fft.rfft2(_ld(x)) * _ld(weights), s=shape)
    raise ValueError(op)


def numpy_f64(op, x, shape, weights=None):
    """The first yardstick: numpy.fft in float64."""
    shape = tuple(int(s) for s in shape)
    if op == "rfft2":
        return np.fft.rfft2(np.asarray(x, np.float64))
    if op == "irfft2":
        return np.fft.irfft2(np.asarray(x, np.complex128), s=shape)
    if op == "fft2":
        return np.fft.fft2(np.asarray(x, np.complex128))
    if op == "ifft2":
        return np.fft.ifft2(np.asarray(x, np.complex128))
    if op == "weighted":
        return np.fft.irfft2(np.fft.rfft2(np.asarray(x, np.float64)) * weights, s=shape)
    raise ValueError(op)


def unit(want):
    """u = 2^-53 x the root mean square of the oracle's output."""
    w = np.asarray(want)
    return float(np.sqrt(np.mean(np.abs(w) ** 2))) * 2.0 ** -53


def compare(got, want):
    """(max |got - oracle| / u, index of the worst bin).  NaN / inf in ``got`` count as an infinite error."""
    want = np.asarray(want)
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(_ld(got) - want)
    err = np.where(np.isfinite(err), err, np.inf)
    at = np.unravel_index(int(np.argmax(err)), err.shape)
    u = unit(want)
    return float(err[at] / u) if u > 0 else (0.0 if err[at] == 0 else float("inf")), tuple(int(i) for i in at)


def rel_l2(got, want):
    """The whole-array bar of tests/test_fft_gpu.py, for the record of what it does not see."""
    want = np.asarray(want)
    den = float(np.sqrt(np.sum(np.abs(want) ** 2)))
    return float(np.sqrt(np.sum(np.abs(_ld(got) - want) ** 2))) / (den if den > 0 else 1.0)


# ---- the kernel's chirp-z transform, restated in float64 ------------------------------------------------------------
def chirp_table(n, reduced=True):
    """b_j, j < n, complex128.  ``reduced``: j^2 mod 2n in integers, the angle in long double, rounded once (make_dft).
    ``reduced=False`` is the seeded defect: pi * j * j / n formed in float64."""
    j = np.arange(n, dtype=np.int64)
    if reduced:
        q =(j * j) % (2 * n)
        pi_ld = np.longdouble("3.14159265358979323846264338327950288")
        a = pi_ld * q.astype(np.longdouble) / np.longdouble(n)
        return (np.cos(a) + 1j * np.sin(a)).astype(np.complex128)
    jf = j.astype(np.float64)
    a = np.pi * jf * jf / float(n)
    return np.cos(a) + 1j * np.sin(a)


def _chirp_axis(x, axis, inverse, reduced=True):
    """Unscaled DFT (inverse: conjugate kernel, still unscaled) of length n along ``axis`` through Bluestein's identity."""
    x = np.moveaxis(np.asarray(x, np.complex128), axis, -1)
    n = x.shape[-1]
    M = 1 << int(np.ceil(np.log2(2 * n - 1)))
    b = chirp_table(n, reduced)
    ext = np.zeros(M, np.complex128)
    ext[:n] = b
    ext[M - n + 1:] = b[:0:-1]
    filt = np.fft.fft(ext)
    if inverse:  # the chirp of the inverse transform is the conjugate one (its extension is symmetric)
        pre, filt, post = b, np.conj(filt), b
    else:
        pre, post = np.conj(b), np.conj(b)
    z = np.zeros(x.shape[:-1] + (M,), np.complex128)
    z[..., :n] = x * pre
    y = np.fft.ifft(np.fft.fft(z, axis=-1) * filt, axis=-1)[..., :n] * post
    return np.moveaxis(y, -1, axis)


def _axis(x, axis, inverse, reduced=True):
    n = x.shape[axis]
    if is_pow2(n):
        return np.fft.ifft(x, axis=axis) * n if inverse else np.fft.fft(x, axis=axis)
    return _chirp_axis(x, axis, inverse, reduced)


def restated(op, x, shape, weights=None, reduced=True):
    """The second yardstick: the kernel's order of passes (rows then columns forward, columns then rows backward) with
    every side that is not a power of two through the float64 chirp-z restatement."""
    m, n = (int(s) for s in shape)
    nc = n // 2 + 1
    if op == "rfft2":
        rows = _axis(np.asarray(x, np.float64).astype(np.complex128), 1, False, reduced)[:, :nc]
        return _axis(rows, 0, False, reduced)
    if op == "fft2":
        return _axis(_axis(np.asarray(x, np.complex128), 1, False, reduced), 0, False, reduced)
    if op == "ifft2":
        return _axis(_axis(np.asarray(x, np.complex128), 1, True, reduced), 0, True, reduced) * (1.0 / (float(m) * float(n)))
    if op == "irfft2":
        cols = _axis(np.asarray(x, np.complex128), 0, True, reduced)
        full = np.zeros((m, n), np.complex128)
        half = cols.copy()
        half[:, 0] = half[:, 0].real  # numpy's rule: the imaginary parts of bin 0 and of the Nyquist bin are dropped
        if n % 2 == 0:
            half[:, nc - 1] = half[:, nc - 1].real
        full[:, :nc] = half
        k = np.arange(1, n - nc + 1)
        full[:, n - k] = np.conj(half[:, k])
        return _axis(full, 1, True, reduced).real * (1.0 / (float(m) * float(n)))
    if op == "weighted":
        return restated("irfft2", restated("rfft2", x, shape, reduced=reduced) * weights, shape, reduced=reduced)
    raise ValueError(op)


# ---- closed forms in long double (the phase reduced exactly in integers before the angle is formed) -----------------
_TWO_PI_LD = 2 * np.longdouble("3.14159265358979323846264338327950288")


def _unit_root(num, den):
    """exp(2 pi i num / den) in long double for integer arrays ``num``: num mod den first."""
    a = _TWO_PI_LD * (np.asarray(num, dtype=np.int64) % int(den)).astype(np.longdouble) / np.longdouble(den)
    return np.cos(a) + 1j * np.sin(a)


def impulse_spectrum(shape, at):
    """fft2 of a unit impulse at ``at``: exp(-2 pi i (k r0 / m + l c0 / n)); every bin has magnitude 1."""
    m, n = shape
    k = np.arange(m, dtype=np.int64)[:, None]
    l = np.arange(n, dtype=np.int64)[None, :]
    return _unit_root(-(k * at[0] * n + l * at[1] * m), m * n)


def tone(shape, at):
    """exp(+2 pi i (k0 r / m + l0 c / n)) in long double: the field whose fft2 is m n at bin ``at`` and zero elsewhere."""
    m, n = shape
    r = np.arange(m, dtype=np.int64)[:, None]
    c = np.arange(n, dtype=np.int64)[None, :]
    return _unit_root(r * at[0] * n + c * at[1] * m, m * n)


# ---- bars -------------------------------------------------------------------------------------------------------------
def load_bars():
    with open(BARS_FILE) as fh:
        return json.load(fh)


def bar(bars, cls, op):
    return float(bars["classes"][cls][op]["bar"])


def case_bar(bars, cls, op, fam):
    """The bar of one case: its class's, and its input family's own where that is smaller (the class's C is set by the
    families whose output holds one spike sqrt(m n) root mean squares large)."""
    entry = bars["classes"][cls][op]
    return min(float(entry["bar"]), float(entry["families"].get(fam, entry)["bar"]))


# ---- the device side (imported lazily: the CPU tests never get here) --------------------------------------------------
def device_op(op, x, shape):
    """One of the four transforms through ``get_hip(shape)``: NumPy in -> NumPy out, DeviceArray in -> DeviceArray out."""
    from pysteps_amd.utils.fft import get_hip

    return getattr(get_hip(tuple(shape)), op)(x)


def device_weighted(field, bank, shape, levels_out=None):
    """``psh_cascade_decompose_levels_dev`` on a host field and a (L, m, n//2+1) bank -> (L, m, n) float64 on the host.
    ``levels_out``: a DeviceArray to write into (the caller reads it back itself)."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    m, n = (int(s) for s in shape)
    d_field = field if isinstance(field, DeviceArray) else DeviceArray.from_host(np.ascontiguousarray(field, np.float64))
    d_bank = DeviceArray.from_host(np.ascontiguousarray(bank, np.float64))
    L = int(bank.shape[0])
    levels = levels_out if levels_out is not None else DeviceArray((L, m, n), np.float64)
    _lib.check(_lib.lib().psh_cascade_decompose_levels_dev(d_field.ptr, d_bank.ptr, L, m, n, levels.ptr),
               "psh_cascade_decompose_levels_dev")
    return None if levels_out is not None else np.array(levels.to_host(), copy=True)
