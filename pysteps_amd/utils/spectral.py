"""Radially averaged power spectra on the device, mirror of ``pysteps.utils.spectral.rapsd`` (reference:
pysteps/utils/spectral.py:100-180).

The reference averages ``|fftshift(fft2(field))|**2 / (m n)`` over the coefficients of every integer radius
``r = round(sqrt(kx**2 + ky**2))`` with one boolean mask of the plane per radius.  Here every bin gathers its own
coefficients (csrc/rapsd.hip): the bin is an integer function of ``kx**2 + ky**2`` (``r**2 - r < N <= r**2 + r``), the
sums are double-double, and the half spectrum of ``rfft2`` with a weight of 2 on the mirrored columns gives the sums and
the integer counts of the full plane.  A bin mean is the exact mean of its terms rounded to float64; the reference's is
``np.mean`` of them.

Served on the device: two-dimensional float32 or float64 fields, NumPy or
:class:`~pysteps_amd.device.DeviceArray`, of a shape :func:`pysteps_amd.utils.fft.supported_shape` takes.  A field
with an infinite value, another shape or another dtype goes to the reference's function with a ``RuntimeWarning`` when
pysteps is importable and the field is a NumPy array, and raises ``NotImplementedError`` otherwise.  ``corrcoef``,
``mean``, ``std`` and ``remove_rain_norain_discontinuity`` of the reference module are single passes over the field and
are not mirrored.
"""

import ctypes

import numpy as np

from .. import _lib
from .._reference import decline, lookup
from ..device import DeviceArray
from . import fft as hip_fft

__all__ = ["rapsd", "rapsd_table", "rapsd_counts", "RapsdAccumulator"]

_BATCH_BYTES = 1 << 30  # half spectra held at a time by the transform path


def _bins(m, n):
    l = max(m, n)
    return l // 2 + (l & 1)


def _freq(m, n, d):
    return np.fft.fftfreq(max(m, n), d=d)[0:_bins(m, n)]


def _is_hip(fft_method):
    return (isinstance(fft_method, str) and fft_method == "hip") or bool(getattr(fft_method, "pysteps_amd_hip", False))


def _why_not(shape, dtype):
    """The reason the device path declines a plane of this shape and dtype, or None."""
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        return "a field of dtype %s" % np.dtype(dtype)
    if not hip_fft.supported_shape(shape):
        return "the shape %s" % (tuple(int(s) for s in shape),)
    return None


def _nonfinite(dev):
    """``(NaN values, infinite values)`` of a float32 or float64 device array."""
    counts = (ctypes.c_ulonglong * 2)()
    _lib.check(_lib.lib().psh_rapsd_nonfinite_dev(dev.ptr, int(dev.dtype == np.float64), dev.size, counts), "psh_rapsd_nonfinite_dev")
    return int(counts[0]), int(counts[1])


def _full(stack):
    """``(means (K, nb), counts (nb,))`` of a device stack ``(K, m, n)`` of shifted power planes."""
    K, m, n = stack.shape
    out, counts = DeviceArray((K, _bins(m, n)), np.float64), DeviceArray((_bins(m, n),), np.uint64)
    _lib.check(_lib.lib().psh_rapsd_full_dev(stack.ptr, int(stack.dtype == np.float64), K, m, n, out.ptr, counts.ptr),
               "psh_rapsd_full_dev")
    return np.array(out.to_host()), np.array(counts.to_host())  # the copies wait for the kernels


def _half(spectra, m, n):
    """``(means (K, nb), counts (nb,))`` of a device stack ``(K, m, n//2+1)`` of complex128 half spectra."""
    K = spectra.shape[0]
    out, counts = DeviceArray((K, _bins(m, n)), np.float64), DeviceArray((_bins(m, n),), np.uint64)
    _lib.check(_lib.lib().psh_rapsd_half_dev(spectra.ptr, K, m, n, out.ptr, counts.ptr), "psh_rapsd_half_dev")
    return np.array(out.to_host()), np.array(counts.to_host())


def _transformed(stack):
    """Means ``(K, nb)`` of a device stack ``(K, m, n)`` of fields: float64 ``rfft2`` of every plane, as many half
    spectra at a time as ``_BATCH_BYTES`` holds, binned as ``psh_fft_rfft2_dev`` wrote them."""
    K, m, n = stack.shape
    nh = n // 2 + 1
    batch = max(1, min(K, _BATCH_BYTES // (m * nh * 16)))
    lib = _lib.lib()
    spectra = DeviceArray((batch, m, nh), np.complex128)
    wide = DeviceArray((m, n), np.float64) if stack.dtype != np.float64 else None
    rows = []
    for k0 in range(0, K, batch):
        count = min(batch, K - k0)
        for j in range(count):
            plane = stack.ptr + (k0 + j) * m * n * stack.dtype.itemsize
            if wide is not None:
                _lib.check(lib.psh_convert_dev(plane, wide.ptr, m * n, 1), "psh_convert_dev")
                plane = wide.ptr
            _lib.check(lib.psh_fft_rfft2_dev(plane, m, n, spectra.ptr + j * m * nh * 16), "psh_fft_rfft2_dev")
        part = spectra if count == batch else DeviceArray((count, m, nh), np.complex128, ptr=spectra.ptr, owner=spectra)
        rows.append(_half(part, m, n)[0])
    return np.concatenate(rows) if len(rows) > 1 else rows[0]


def _host_power(field, fft_method, fft_kwargs):
    """The reference's own expression for the shifted power plane, on the host."""
    psd = fft_method.fftshift(fft_method.fft2(field, **fft_kwargs))
    psd = np.abs(psd) ** 2 / psd.size
    if psd.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        psd = psd.astype(np.float64)
    return np.ascontiguousarray(psd)


def _spectra(fields, fft_method, fft_kwargs):
    """Means ``(K, nb)`` of a stack ``(K, m, n)``, NumPy or resident, of a served shape and dtype; None when a value is
    infinite.  A NaN raises the reference's error."""
    resident = isinstance(fields, DeviceArray)
    dev = fields if resident else DeviceArray.from_host(np.ascontiguousarray(fields))
    nans, infs = _nonfinite(dev)
    if nans:
        raise ValueError("input field should not contain nans")
    if infs:
        return None
    if fft_method is None:
        return _full(dev)[0]
    if _is_hip(fft_method):
        return _transformed(dev)
    host = dev.to_host() if resident else np.asarray(fields)
    power = np.stack([_host_power(plane, fft_method, fft_kwargs) for plane in host])
    return _full(DeviceArray.from_host(power))[0]


def rapsd(field, fft_method=None, return_freq=False, d=1.0, normalize=False, **fft_kwargs):
    """Compute radially averaged power spectral density (RAPSD) from the given 2D input field; the signature, the two
    ``ValueError`` s (dimension count, NaN), the return shapes and ``freq`` are the reference's.

    ``field`` is ``(m, n)``, a NumPy array or a DeviceArray of float32 or float64 (a resident float32 field is widened
    on the device).  ``fft_method`` chooses the path: ``None`` - ``field`` is the shifted power plane itself and is
    binned as it is; the object of :func:`pysteps_amd.utils.fft.get_hip` or the string ``"hip"`` - float64 ``rfft2`` on
    the device, binned from the half spectrum, nothing leaves HBM but the ``nb`` means (``fft_kwargs`` are ignored);
    any other object, such as ``np.fft`` - the reference's expression ``fftshift(fft2(field))`` on the host, binned on
    the device.  Where the reference's function runs in place of the device path (module docstring), ``"hip"`` stands
    for ``np.fft``, the reference's default method.  ``normalize`` divides by the sum of the result, ``return_freq`` also returns
    ``np.fft.fftfreq(l, d)[0:nb]`` with ``l = max(m, n)`` and ``nb = l // 2`` (``+ 1`` for odd ``l``).

    The result is always float64: with NumPy >= 2 the reference returns float32 for a float32 field through
    ``np.fft``; here the float32 power is averaged as its float64 values."""
    if len(field.shape) != 2:
        raise ValueError(f"{len(field.shape)} dimensions are found, but the number of dimensions should be 2")
    resident = isinstance(field, DeviceArray)
    if not resident:
        field = np.asanyarray(field)
    why = _why_not(field.shape, field.dtype)
    result = None
    if why is None:
        stack = DeviceArray((1,) + field.shape, field.dtype, ptr=field.ptr, owner=field) if resident else field[np.newaxis]
        result = _spectra(stack, fft_method, fft_kwargs)
        why = "an infinite value" if result is None else None
    if why is not None:
        # the reference calls fft_method.fft2 / .fftshift: the string "hip" stands for its default method there
        method = np.fft if isinstance(fft_method, str) else fft_method
        return decline("rapsd", why, lookup("utils.spectral", "rapsd", rapsd), resident)(
            field, fft_method=method, return_freq=return_freq, d=d, normalize=normalize, **fft_kwargs)
    result = result[0]
    if normalize:
        result /= np.sum(result)
    if return_freq:
        return result, _freq(field.shape[0], field.shape[1], d)
    return result


def rapsd_table(fields, fft_method="hip", normalize=False, return_freq=False, d=1.0):
    """The spectra of a stack ``(K, m, n)``, NumPy or DeviceArray, from one call: float64 ``(K, nb)``, row ``k`` equal
    to ``rapsd(fields[k], fft_method, normalize=normalize)`` bit for bit (the kernels' sums do not depend on ``K`` or on
    where a plane lies).  With the device transform every plane is transformed by a call of its own into a buffer of
    half spectra that fits ``_BATCH_BYTES``; the binning takes the buffer in one launch.  With ``return_freq`` returns ``(table, freq)``."""
    if len(fields.shape) != 3:
        raise ValueError("rapsd_table: fields of shape (K, m, n) expected, got %s" % (tuple(fields.shape),))
    resident = isinstance(fields, DeviceArray)
    if not resident:
        fields = np.asanyarray(fields)
    K, m, n = fields.shape
    if K < 1:
        raise ValueError("rapsd_table: no field given")
    why = _why_not((m, n), fields.dtype)
    table = _spectra(fields, fft_method, {}) if why is None else None
    if table is None:
        if resident:
            decline("rapsd_table", why or "an infinite value", lookup("utils.spectral", "rapsd", rapsd), True)
        table = np.stack([rapsd(fields[k], fft_method=fft_method) for k in range(K)])  # declines plane by plane
    if normalize:
        for k in range(K):
            table[k] /= np.sum(table[k])
    if return_freq:
        return table, _freq(m, n, d)
    return table


def rapsd_counts(shape, half=False):
    """The number of coefficients of every bin of a ``(m, n)`` plane, int64 ``(nb,)``, counted on the device: over the
    shifted full plane, or with ``half=True`` over the half spectrum with its weights - the same integers."""
    m, n = (int(s) for s in shape)
    counts = DeviceArray((_bins(m, n),), np.uint64)
    _lib.check(_lib.lib().psh_rapsd_counts_dev(m, n, 0 if half else 1, counts.ptr), "psh_rapsd_counts_dev")
    return counts.to_host().astype(np.int64)


class RapsdAccumulator:
    """Power spectra of a nowcast where its members lie, usable as the ``callback`` of a nowcast::

        acc = RapsdAccumulator(observations)
        nowcasts.get_method("steps")(..., callback=acc, return_output=False)
        acc.mean_spectra           # (n_leadtimes, nb): the members' mean spectrum per lead time
        acc.ratio()                # ... over the spectrum of the observation of that lead time
        acc.freq(d=1.0)            # the frequencies of the nb bins

    Call ``t`` receives the members of lead time ``t`` - a ``DeviceArray`` ``(k, m, n)`` from the resident nowcast loop, a
    host ``ndarray`` from any other - and takes every member's spectrum through the device transform
    (:func:`rapsd_table`).  ``observations``, when given, is ``(n_leadtimes, m, n)``, NumPy or DeviceArray, and is kept
    on the device; its spectra are ``obs_spectra``.  ``normalize`` normalizes every spectrum before it is averaged.
    ``per_member=True`` also keeps every member's own spectrum (``member_spectra``).  A NaN in a field raises as
    :func:`rapsd` does unless ``nan_value`` is given: every NaN pixel then takes that value first (the zero value of the
    transformed field, for the pixels a nowcast has advected in from outside)."""

    accepts_device = True

    def __init__(self, observations=None, normalize=False, per_member=False, nan_value=None):
        self.normalize, self.per_member, self.nan_value = bool(normalize), bool(per_member), nan_value
        self._obs = None
        self._shape = None
        self._obs_spectra = None
        if observations is not None:
            if len(observations.shape) != 3:
                raise ValueError("RapsdAccumulator: observations of shape (n_leadtimes, m, n) expected, got %s"
                                 % (tuple(observations.shape),))
            self._obs = observations if isinstance(observations, DeviceArray) else DeviceArray.from_host(np.asarray(observations))
            self._shape = self._obs.shape[1:]
            self._obs_spectra = rapsd_table(self._filled(self._obs), "hip", normalize=self.normalize)
        self._mean = []
        self._members = []
        self.n_leadtimes = 0
        self.received = []  # type of the members of every call: DeviceArray or ndarray

    def _filled(self, stack):
        if self.nan_value is None:
            return stack
        if _why_not(stack.shape[1:], stack.dtype) is not None:  # declined further on: filled on the host, if at all
            if isinstance(stack, DeviceArray) or stack.dtype.kind != "f":
                return stack
            return np.where(np.isnan(stack), stack.dtype.type(self.nan_value), stack)
        dev = stack if isinstance(stack, DeviceArray) else DeviceArray.from_host(np.ascontiguousarray(stack))
        out = DeviceArray(dev.shape, np.float64)
        _lib.check(_lib.lib().psh_rapsd_fill_nan_dev(dev.ptr, int(dev.dtype == np.float64), dev.size, float(self.nan_value), out.ptr),
                   "psh_rapsd_fill_nan_dev")
        return out

    def __call__(self, members):
        resident = isinstance(members, DeviceArray)
        self.received.append(DeviceArray if resident else np.ndarray)
        if not resident:
            members = np.asarray(members)
        if len(members.shape) != 3 or (self._shape is not None and tuple(members.shape[1:]) != self._shape):
            expected = "(k, %d, %d)" % self._shape if self._shape is not None else "(k, m, n)"
            raise ValueError("RapsdAccumulator: members of shape %s expected, got %s" % (expected, tuple(members.shape)))
        if self._obs is not None and self.n_leadtimes >= self._obs.shape[0]:
            raise ValueError("RapsdAccumulator: called for more lead times than the %d observations" % self._obs.shape[0])
        self._shape = tuple(members.shape[1:])
        table = rapsd_table(self._filled(members), "hip", normalize=self.normalize)
        self._mean.append(np.mean(table, axis=0))
        if self.per_member:
            self._members.append(table)
        self.n_leadtimes += 1

    @property
    def mean_spectra(self):
        """float64 ``(n_leadtimes, nb)``: the mean over the members of their spectra, per lead time; None before the
        first call."""
        return np.stack(self._mean) if self._mean else None

    @property
    def member_spectra(self):
        """With ``per_member=True`` the list, per lead time, of the members' spectra ``(k, nb)``, else None."""
        return list(self._members) if self._members else None

    @property
    def obs_spectra(self):
        """float64 ``(n_leadtimes, nb)``: the spectra of the observations, or None when none were given."""
        return self._obs_spectra

    def freq(self, d=1.0):
        """The Fourier frequencies of the bins for the sample spacing ``d``, as ``rapsd(return_freq=True)`` returns them."""
        if self._shape is None:
            raise ValueError("RapsdAccumulator: no field seen yet")
        return _freq(self._shape[0], self._shape[1], d)

    def ratio(self):
        """``mean_spectra`` over the spectra of the observations of the lead times seen so far, ``(n_leadtimes, nb)``:
        below 1 where the ensemble has lost power at that scale."""
        if self._obs_spectra is None:
            raise ValueError("RapsdAccumulator: no observations given")
        if not self._mean:
            raise ValueError("RapsdAccumulator: no field seen yet")
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.mean_spectra / self._obs_spectra[: self.n_leadtimes]
