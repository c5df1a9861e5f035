"""Transforms on the device, mirror of pysteps/utils/transformation.py (``boxcox_transform``, ``dB_transform``,
``NQ_transform``, ``sqrt_transform``).

NumPy inputs are transformed on the host exactly like the reference does (it is one
element-wise pass); :class:`~pysteps_amd.device.DeviceArray` inputs stay in HBM
(``psh_db_transform_dev``) so that rain rate -> dB -> LK -> extrapolation -> rain rate
never crosses PCIe.
"""

import ctypes

import numpy as np

from .. import _lib
from ..device import DeviceArray, _compared_as

__all__ = ["dB_transform", "boxcox_transform", "NQ_transform", "sqrt_transform", "ResidentInterp", "field_stats",
           "field_nanmin"]


def _require_float32(field):
    if field.dtype != np.float32:
        raise ValueError("device-resident fields must be float32")


def _field_stats(field):
    _require_float32(field)
    mn, mx, bad, low = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    _lib.check(
        _lib.lib().psh_field_stats_dev(field.ptr, field.size, ctypes.byref(mn), ctypes.byref(mx), ctypes.byref(bad),
                                       ctypes.byref(low)),
        "psh_field_stats_dev",
    )
    return mn.value, mx.value, int(bad.value), low.value


def field_stats(field):
    """(min, max, number of non-finite values) of a float32 DeviceArray, computed on the device;
    min and max are over the finite values."""
    return _field_stats(field)[:3]


def field_nanmin(field):
    """``np.nanmin`` of a float32 DeviceArray from the same device reduction: NaNs are ignored, an
    infinity is a value (semilagrangian.py:171-172, outval="min")."""
    return _field_stats(field)[3]


def _transform_dev(R, compared_with, zerovalue, inverse):
    """One resident pass.  ``compared_with`` is the threshold object of the reference's ``<``, in the
    units of the values it is compared with; it decides in float32 or in float64 as NumPy would."""
    _require_float32(R)
    out = DeviceArray(R.shape, np.float32)
    _lib.check(_lib.lib().psh_db_transform_dev(R.ptr, out.ptr, R.size, _compared_as(compared_with, np.float32),
                                               float(zerovalue), int(inverse)), "psh_db_transform_dev")
    return out


def dB_transform(R, metadata=None, threshold=None, zerovalue=None, inverse=False):
    """Methods to transform precipitation intensities to/from dB units.

    Same parameters, return value ``(R, metadata)`` and metadata updates as the
    reference (transformation.py:150-232).
    """
    if metadata is None:
        metadata = {"transform": "dB"} if inverse else {"transform": None}
    else:
        metadata = metadata.copy()
    on_device = isinstance(R, DeviceArray)

    if not inverse:
        if metadata["transform"] == "dB":
            return (R if on_device else R.copy()), metadata
        if threshold is None:
            threshold = metadata.get("threshold", 0.1)
        threshold_db = 10.0 * np.log10(threshold)
        if zerovalue is None:
            zerovalue = threshold_db - 5
        if on_device:
            out = _transform_dev(R, threshold, zerovalue, False)
        else:
            out = R.copy()
            zeros = out < threshold
            out[~zeros] = 10.0 * np.log10(out[~zeros])
            out[zeros] = zerovalue
        metadata["transform"] = "dB"
        metadata["zerovalue"] = zerovalue
        metadata["threshold"] = threshold_db
        return out, metadata

    if metadata["transform"] != "dB":
        return (R if on_device else R.copy()), metadata
    if threshold is None:
        threshold = metadata.get("threshold", -10.0)
    if zerovalue is None:
        zerovalue = 0.0
    # formed as the reference forms it (:227), so it keeps the NumPy type that decides the comparison: the
    # metadata of a forward transform holds a numpy.float64, a Python float stays a Python float
    threshold_lin = 10.0 ** (threshold / 10.0)
    if on_device:
        out = _transform_dev(R, threshold_lin, zerovalue, True)
    else:
        out = 10.0 ** (R / 10.0)
        out[out < threshold_lin] = zerovalue
    metadata["transform"] = None
    metadata["threshold"] = threshold_lin
    metadata["zerovalue"] = zerovalue
    return out, metadata


# ---- Box-Cox, square root, normal quantiles -----------------------------------------------------------------------------

# operations of psh_field_transform_dev (include/pysteps_hip.h)
OP_BOXCOX, OP_BOXCOX_INVERSE, OP_SQRT, OP_SQUARE, OP_Z_TO_RATE, OP_RATE_TO_Z = range(6)
NQT_MAX_VALUES = 2 ** 32 - 1  # counts and sort positions are uint32


def _ref(name):
    """The reference's function of that name, or None (looked up only once a call has been declined)."""
    from .._reference import lookup

    if name in globals():
        return lookup("utils.transformation", name, globals()[name])
    return lookup("utils.conversion", name, None)


def _resident_real(name, R, *scalars):
    """A resident field the element-wise passes take: float32 or float64, and scalars that leave NumPy's result in that
    dtype (a numpy.float64 parameter would widen a float32 field in the reference)."""
    from .._reference import decline

    if R.dtype not in (np.float32, np.float64):
        decline(name, "a field of dtype %s" % R.dtype, _ref(name), True)
    for x in scalars:
        if np.result_type(R.dtype, x) != R.dtype:
            decline(name, "a %s parameter with a %s field" % (type(x).__name__, R.dtype), _ref(name), True)


def _pass_dev(R, op, p0=0.0, p1=0.0, compared_with=0.0, zerovalue=0.0):
    out = DeviceArray(R.shape, R.dtype)
    _lib.check(_lib.lib().psh_field_transform_dev(R.ptr, out.ptr, int(R.dtype == np.float32), R.size, op, float(p0), float(p1),
                                                  _compared_as(compared_with, R.dtype), float(zerovalue)),
               "psh_field_transform_dev")
    return out


def boxcox_transform(R, metadata=None, Lambda=None, threshold=None, zerovalue=None, inverse=False):
    """The one-parameter Box-Cox transformation: ``ln(x)`` for ``Lambda == 0``, else ``(x ** Lambda - 1) / Lambda``.

    Same parameters, return value ``(R, metadata)`` and metadata updates as the reference (transformation.py:27-147).
    """
    if metadata is None:
        metadata = {"transform": "BoxCox"} if inverse else {"transform": None}
    else:
        metadata = metadata.copy()
    on_device = isinstance(R, DeviceArray)

    if not inverse:
        if metadata["transform"] == "BoxCox":
            return (R if on_device else R.copy()), metadata
        if Lambda is None:
            Lambda = metadata.get("BoxCox_lambda", 0.0)
        if threshold is None:
            threshold = metadata.get("threshold", 0.1)
        # the transformed threshold keeps the type these expressions give it: it decides a later comparison
        if Lambda == 0.0:
            threshold_t = np.log(threshold)
        else:
            threshold_t = (threshold ** Lambda - 1) / Lambda
        if zerovalue is None:
            zerovalue = threshold_t - 1
        if on_device:
            _resident_real("boxcox_transform", R, Lambda)
            out = _pass_dev(R, OP_BOXCOX, Lambda, 0.0, threshold, zerovalue)
        else:
            out = R.copy()
            zeros = out < threshold
            out[~zeros] = np.log(out[~zeros]) if Lambda == 0.0 else (out[~zeros] ** Lambda - 1) / Lambda
            out[zeros] = zerovalue
        metadata["transform"] = "BoxCox"
        metadata["BoxCox_lambda"] = Lambda
        metadata["zerovalue"] = zerovalue
        metadata["threshold"] = threshold_t
        return out, metadata

    if metadata["transform"] not in ["BoxCox", "log"]:
        return (R if on_device else R.copy()), metadata
    if Lambda is None:
        Lambda = metadata.pop("BoxCox_lambda", 0.0)
    if threshold is None:
        threshold = metadata.get("threshold", -10.0)
    if zerovalue is None:
        zerovalue = 0.0
    if Lambda == 0.0:
        threshold_lin = np.exp(threshold)
    else:
        threshold_lin = np.exp(np.log(Lambda * threshold + 1) / Lambda)
    if on_device:
        _resident_real("boxcox_transform", R, Lambda)
        out = _pass_dev(R, OP_BOXCOX_INVERSE, Lambda, 0.0, threshold_lin, zerovalue)
    else:
        out = np.exp(R) if Lambda == 0.0 else np.exp(np.log(Lambda * R + 1) / Lambda)
        out[out < threshold_lin] = zerovalue
    metadata["transform"] = None
    metadata["zerovalue"] = zerovalue
    metadata["threshold"] = threshold_lin
    return out, metadata


def sqrt_transform(R, metadata=None, inverse=False, **kwargs):
    """Square-root transform; same parameters, return value and metadata updates as the reference
    (transformation.py:329-380): without metadata the zerovalue and the threshold become NaN."""
    if metadata is None:
        metadata = {"transform": "sqrt" if inverse else None, "zerovalue": np.nan, "threshold": np.nan}
    else:
        metadata = metadata.copy()
    on_device = isinstance(R, DeviceArray)
    if on_device:
        _resident_real("sqrt_transform", R)
    if not inverse:
        out = _pass_dev(R, OP_SQRT) if on_device else np.sqrt(R)
        metadata["transform"] = "sqrt"
        metadata["zerovalue"] = np.sqrt(metadata["zerovalue"])
        metadata["threshold"] = np.sqrt(metadata["threshold"])
    else:
        out = _pass_dev(R, OP_SQUARE) if on_device else R ** 2
        metadata["transform"] = None
        metadata["zerovalue"] = metadata["zerovalue"] ** 2
        metadata["threshold"] = metadata["threshold"] ** 2
    return out, metadata


def _plotting_positions(n, a):
    return (np.arange(n) + 1 - a) / (n + 1 - 2 * a)


def _f32_flag(dtype):
    return int(np.dtype(dtype) == np.float32)


class ResidentInterp:
    """``metadata["inqt"]`` of a resident forward ``NQ_transform``: the sorted values on the device with ``n`` and ``a``.

    Called on a :class:`DeviceArray` it evaluates ``scipy.interpolate.interp1d``'s linear rule on the device
    (``psh_nqt_inverse_dev``) against the quantile table ``psh_nqt_table_dev`` makes on first use; called on a NumPy
    array it is the ``interp1d`` the reference would have built from the same values.
    """

    def __init__(self, sorted_dev, n, a, rqn_dev=None):
        self.sorted_dev, self.n, self.a, self._rqn_dev, self._host = sorted_dev, int(n), a, rqn_dev, None

    @classmethod
    def from_interp1d(cls, f):
        """The tables of a real ``interp1d`` made by the reference's forward transform, uploaded."""
        x, y = np.asarray(f.x, np.float64), np.asarray(f.y, np.float64)
        fill = f.fill_value if isinstance(f.fill_value, tuple) else (f.fill_value, f.fill_value)
        if x.ndim != 1 or y.shape != x.shape or x.size < 2 or getattr(f, "bounds_error", False) \
                or np.ravel(fill[0])[0] != y[0] or np.ravel(fill[1])[0] != y[-1] or not np.all(np.diff(x) > 0):
            raise NotImplementedError("pysteps_amd NQ_transform: this interp1d is not one the forward transform builds")
        return cls(DeviceArray.from_host(y), x.size, None, DeviceArray.from_host(x))

    def table(self):
        """The quantile table Rqn (n float64) on the device."""
        if self._rqn_dev is None:
            rqn = DeviceArray((self.n,), np.float64)
            _lib.check(_lib.lib().psh_nqt_table_dev(self.n, float(self.a), rqn.ptr), "psh_nqt_table_dev")
            self._rqn_dev = rqn
        return self._rqn_dev

    def evaluate_dev(self, x, dtype=None):
        """(result, its minimum, the smallest value above the minimum) for a resident ``x``."""
        if x.dtype not in (np.float32, np.float64) or x.size == 0:
            raise NotImplementedError("pysteps_amd NQ_transform: resident fields are float32 or float64 and not empty")
        out = DeviceArray(x.shape, np.float64 if dtype is None else dtype)
        lowest, above = ctypes.c_double(), ctypes.c_double()
        _lib.check(_lib.lib().psh_nqt_inverse_dev(x.ptr, _f32_flag(x.dtype), x.size, self.table().ptr, self.sorted_dev.ptr,
                                                  _f32_flag(self.sorted_dev.dtype), self.n, out.ptr, _f32_flag(out.dtype),
                                                  ctypes.byref(lowest), ctypes.byref(above)), "psh_nqt_inverse_dev")
        return out, lowest.value, above.value

    def __call__(self, x):
        if isinstance(x, DeviceArray):
            return self.evaluate_dev(x)[0]
        if self._host is None:
            from scipy.interpolate import interp1d
            from scipy.stats import norm

            ys = self.sorted_dev.to_host(out=np.empty(self.sorted_dev.shape, self.sorted_dev.dtype))[:self.n].astype(float)
            xs = self._rqn_dev.to_host(out=np.empty((self.n,), np.float64)) if self.a is None else norm.ppf(
                _plotting_positions(self.n, self.a))
            self._host = interp1d(xs, ys, bounds_error=False, fill_value=(ys[0], ys[-1]))
        return self._host(x)


_EMPTY_MIN = "zero-size array to reduction operation minimum which has no identity"


def _nq_resident(R, metadata, inverse, a, dtype):
    from .._reference import decline

    if R.dtype not in (np.float32, np.float64):
        decline("NQ_transform", "a field of dtype %s" % R.dtype, _ref("NQ_transform"), True)
    if R.size > NQT_MAX_VALUES:
        decline("NQ_transform", "more than 2^32 - 1 values", _ref("NQ_transform"), True)
    if dtype is not None and np.dtype(dtype) not in (np.float32, np.float64):
        raise ValueError("NQ_transform: dtype must be float32 or float64")
    if R.size == 0:
        raise ValueError(_EMPTY_MIN)
    lib = _lib.lib()
    out_dtype = np.float64 if dtype is None else np.dtype(dtype)
    if inverse:
        # the reference takes np.min of the input for a missing metadata and overwrites it below: nothing to compute
        metadata = {"transform": "NQT", "zerovalue": None} if metadata is None else metadata.copy()
        f = metadata.pop("inqt")
        if not isinstance(f, ResidentInterp):
            f = ResidentInterp.from_interp1d(f)
        out, lowest, above = f.evaluate_dev(R, out_dtype)
        if lowest != lowest or above != above:
            raise ValueError(_EMPTY_MIN)
        metadata["transform"] = None
        metadata["zerovalue"] = np.float64(lowest)
        metadata["threshold"] = np.float64(above)
        return out, metadata

    count = DeviceArray(R.shape, np.uint32)
    ordered = DeviceArray((R.size,), R.dtype)
    n_valid, lowest, highest = ctypes.c_size_t(), ctypes.c_double(), ctypes.c_double()
    _lib.check(lib.psh_nqt_count_le_dev(R.ptr, _f32_flag(R.dtype), R.size, count.ptr, ordered.ptr, ctypes.byref(n_valid),
                                        ctypes.byref(lowest), ctypes.byref(highest), None), "psh_nqt_count_le_dev")
    n = n_valid.value
    if n == 0:
        raise ValueError(_EMPTY_MIN)
    if np.isinf(lowest.value) or np.isinf(highest.value):
        decline("NQ_transform", "a field with infinite values", _ref("NQ_transform"), True)
    if metadata is None:
        metadata = {"transform": None, "zerovalue": np.float64(lowest.value)}
    else:
        metadata = metadata.copy()
    out = DeviceArray(R.shape, out_dtype)
    smallest = ctypes.c_double()
    _lib.check(lib.psh_nqt_forward_dev(R.ptr, _f32_flag(R.dtype), count.ptr, R.size, n, float(a), float(metadata["zerovalue"]),
                                       out.ptr, _f32_flag(out_dtype), ctypes.byref(smallest)), "psh_nqt_forward_dev")
    if smallest.value != smallest.value:
        raise ValueError(_EMPTY_MIN)
    metadata["inqt"] = ResidentInterp(ordered, n, a)
    metadata["transform"] = "NQT"
    metadata["zerovalue"] = 0
    metadata["threshold"] = np.float64(smallest.value)
    return out, metadata


def NQ_transform(R, metadata=None, inverse=False, *, dtype=None, **kwargs):
    """The normal quantile transformation as in Bogner et al. (2012); zero rain becomes zero in normal space.

    Same parameters (``a`` among ``kwargs``), return value ``(R, metadata)`` and metadata updates as the reference
    (transformation.py:237-326); the result is float64 whatever the input.  ``dtype=np.float32``, the one addition,
    rounds each result once at the store; the thresholds in the metadata are then those of the stored values.
    For a resident field ``metadata["inqt"]`` is a :class:`ResidentInterp`; the inverse accepts that or an ``interp1d``.
    """
    a = kwargs.get("a", 0.0)
    if isinstance(R, DeviceArray):
        return _nq_resident(R, metadata, inverse, a, dtype)

    from .._reference import decline, lookup

    R = np.asarray(R)
    why = None
    if R.dtype not in (np.float32, np.float64):
        why = "a field of dtype %s" % R.dtype
    elif R.size > NQT_MAX_VALUES:
        why = "more than 2^32 - 1 values"
    elif np.isinf(R).any():
        why = "a field with infinite values"
    if why is not None:
        return decline("NQ_transform", why, lookup("utils.transformation", "NQ_transform", NQ_transform), False)(
            R, metadata, inverse, **kwargs)

    from scipy.interpolate import interp1d
    from scipy.stats import norm

    shape = R.shape
    flat = R.ravel().astype(float)
    is_nan = np.isnan(flat)
    values = flat[~is_nan]
    if metadata is None:
        metadata = {"transform": "NQT" if inverse else None, "zerovalue": np.min(values)}
    else:
        metadata = metadata.copy()
    if not inverse:
        rqn = norm.ppf(_plotting_positions(values.size, a))
        ordered = values[np.argsort(values)]
        result = np.interp(values, ordered, rqn)
        result[values == metadata["zerovalue"]] = 0
        metadata["inqt"] = interp1d(rqn, ordered, bounds_error=False, fill_value=(values.min(), values.max()))
        if dtype is not None:
            result = result.astype(dtype)
        metadata["transform"] = "NQT"
        metadata["zerovalue"] = 0
        metadata["threshold"] = np.float64(result[result > 0].min())
    else:
        f = metadata.pop("inqt")
        result = f(values)
        if dtype is not None:
            result = result.astype(dtype)
        metadata["transform"] = None
        metadata["zerovalue"] = np.float64(result.min())
        metadata["threshold"] = np.float64(result[result > result.min()].min())
    out = np.full(flat.shape, np.nan, result.dtype)
    out[~is_nan] = result
    return out.reshape(shape), metadata
