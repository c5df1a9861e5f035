"""Aggregation in time and space, clipping and squaring of the domain: mirror of pysteps/utils/dimension.py
(``aggregate_fields`` :219-339, ``aggregate_fields_time`` :25-117, ``aggregate_fields_space`` :120-216, ``clip_domain``
:342-451, ``square_domain`` :454-599) - signatures, defaults, early returns, metadata updates and exception texts in the
reference's order.

NumPy input runs the reference's NumPy operations on the host and returns NumPy.  A
:class:`~pysteps_amd.device.DeviceArray` goes through csrc/dimension.hip and returns a ``DeviceArray``; the field never
touches the host (``square_domain(method="pad")`` reads one number back, the field's minimum).  float32 and float64 are
served on the device, other resident dtypes raise ``NotImplementedError``.

The aggregations carry the reference's bits: NumPy reduces the ``(k, w, P)`` view along axis 1 in index order, starting
from +0 (so a window of -0.0 gives +0.0), and a thread of the kernels does the same for its output element.  The one
case in which NumPy adds in another order - every other dimension has extent 1 and the window holds at least 8 entries,
where it sums pairwise - is not served on the device and raises ``NotImplementedError`` for resident input.

``clip_domain`` and ``square_domain`` take one keyword more than the reference, ``dtype``: the reference returns float64
wherever it builds the result with ``np.ones`` / ``np.zeros``; ``dtype=np.float32`` stores float32 instead, so that the
result can go straight into the float32 motion and advection kernels.

Where the minimum of a field is a zero and zeros of both signs occur, the sign of ``square_domain``'s pad value follows
the traversal order of ``numpy.min`` on the host and of the reduction on the device; they need not agree.

:class:`TimeAggregator` is the running form of ``aggregate_fields_time`` for the ``callback`` of a nowcast.
"""

import ctypes

import numpy as np

from .. import _lib
from ..device import DeviceArray

__all__ = ["aggregate_fields", "aggregate_fields_time", "aggregate_fields_space", "clip_domain", "square_domain",
           "TimeAggregator"]

_aggregation_methods = dict(sum=np.sum, mean=np.mean, nanmean=np.nanmean, nansum=np.nansum)
_METHOD_CODES = {"sum": 0, "mean": 1, "nansum": 2, "nanmean": 3}  # PSH_AGG_* of include/pysteps_hip_dimension.h
_ROUTES = {"auto": 0, "fused": 1, "two_launch": 2}  # PSH_SPACE_*
_NATIVE = (np.dtype(np.float32), np.dtype(np.float64))
PAIRWISE_FROM = 8  # NumPy's pairwise summation starts at 8 entries of a contiguous run


def _resident_real(what, R):
    if R.dtype not in _NATIVE:
        raise NotImplementedError("%s on the device: float32 or float64 fields, not %s" % (what, R.dtype))


def _copy(R):
    """``R.copy()``."""
    if not isinstance(R, DeviceArray):
        return R.copy()
    out = DeviceArray(R.shape, R.dtype)
    if R.nbytes:
        _lib.check(_lib.lib().psh_memcpy_d2d(out.ptr, R.ptr, R.nbytes), "psh_memcpy_d2d")
    out._keep = (R, R._keep)
    return out


def _own(R):
    """The reference's opening ``R.copy()``.  A resident field is not copied here: nothing below writes into it, and
    :func:`_returned` copies where the input itself would be handed back."""
    return R if isinstance(R, DeviceArray) else R.copy()


def _returned(R):
    return _copy(R) if isinstance(R, DeviceArray) else R


def _reshaped(R, shape):
    """The same device memory under another shape."""
    out = DeviceArray(shape, R.dtype, ptr=R.ptr, owner=R)
    assert out.size == R.size
    return out


def _squeezed(R):
    if not isinstance(R, DeviceArray):
        return R.squeeze()
    return _reshaped(R, tuple(s for s in R.shape if s != 1))


def _refuse_pairwise(shape, axis, window_size):
    others = int(np.prod(shape[:axis], dtype=np.int64)) * int(np.prod(shape[axis + 1:], dtype=np.int64))
    if others == 1 and window_size >= PAIRWISE_FROM:
        raise NotImplementedError(
            "aggregate_fields on the device: every other dimension has extent 1 and the window holds %d >= %d entries; "
            "NumPy sums such a window pairwise, and that order is not implemented on the device" % (window_size, PAIRWISE_FROM))


def _check_window(shape, axis, window_size, trim):
    """The reference's checks of one window against one axis (dimension.py:313-322)."""
    if window_size <= 0:
        raise ValueError("'window_size' must be strictly positive")
    if (shape[axis] % window_size) and (not trim):
        raise ValueError(
            f"Since 'trim' argument was set to False,"
            f"the 'window_size' {window_size} must exactly divide"
            f"the dimension along the selected axis:"
            f"data.shape[axis]={shape[axis]}"
        )


def _aggregate_axis_dev(data, window_size, axis, method, trim):
    shape = data.shape
    axis = int(axis)
    if axis < 0:
        axis += len(shape)
    window_size = int(window_size)
    _resident_real("aggregate_fields", data)
    _refuse_pairwise(shape, axis, window_size)
    pre = int(np.prod(shape[:axis], dtype=np.int64))
    post = int(np.prod(shape[axis + 1:], dtype=np.int64))
    out = DeviceArray(shape[:axis] + (shape[axis] // window_size,) + shape[axis + 1:], data.dtype)
    _lib.check(_lib.lib().psh_aggregate_axis_dev(data.ptr, int(data.dtype == np.float64), pre, shape[axis], post, window_size,
                                                 _METHOD_CODES[method], int(bool(trim)), out.ptr), "psh_aggregate_axis_dev")
    out._keep = (data, data._keep)
    return out


def aggregate_fields(data, window_size, axis=0, method="mean", trim=False):
    """Aggregate ``data`` along ``axis`` in windows of ``window_size``; parameters and return value as documented in the
    reference (dimension.py:219-268).  The result keeps the dtype."""
    if np.ndim(axis) > 1:
        raise TypeError("Only integers or integer 1D arrays can be used for the " "'axis' argument.")

    if np.ndim(axis) == 1:
        axis = np.asarray(axis)
        if np.ndim(window_size) == 0:
            window_size = (window_size,) * axis.size
        window_size = np.asarray(window_size, dtype="int")
        if window_size.shape != axis.shape:
            raise ValueError(
                "The 'window_size' and 'axis' shapes are incompatible."
                f"window_size.shape: {str(window_size.shape)}, "
                f"axis.shape: {str(axis.shape)}, "
            )
        new_data = data if (isinstance(data, DeviceArray) and axis.size) else _copy(data)  # every pass makes a new array
        for i in range(axis.size):
            new_data = aggregate_fields(new_data, window_size[i], axis=axis[i], method=method, trim=trim)
        return new_data

    if np.ndim(window_size) != 0:
        raise TypeError(
            "A single axis was selected for the aggregation but several" f"of window_sizes were given: {str(window_size)}."
        )

    resident = isinstance(data, DeviceArray)
    if not resident:
        data = np.asarray(data).copy()
    orig_shape = data.shape

    if method not in _aggregation_methods:
        raise ValueError(
            "Aggregation method not recognized. " f"Available methods: {str(list(_aggregation_methods.keys()))}"
        )
    _check_window(orig_shape, axis, window_size, trim)

    if resident:
        return _aggregate_axis_dev(data, window_size, axis, method, trim)

    new_data = data.swapaxes(axis, 0)
    if trim:
        trim_size = data.shape[axis] % window_size
        if trim_size > 0:
            new_data = new_data[:-trim_size]
    new_data_shape = list(new_data.shape)
    new_data_shape[0] //= window_size
    new_data = new_data.reshape(new_data_shape[0], window_size, -1)
    new_data = _aggregation_methods[method](new_data, axis=1)
    return new_data.reshape(new_data_shape).swapaxes(axis, 0)


def aggregate_fields_time(R, metadata, time_window_min, ignore_nan=False):
    """Aggregate fields in time; parameters, return value and metadata updates of the reference (dimension.py:25-117)."""
    R = _own(R)
    metadata = metadata.copy()

    if time_window_min is None:
        return _returned(R), metadata

    unit = metadata["unit"]
    timestamps = metadata["timestamps"]
    if "leadtimes" in metadata:
        leadtimes = metadata["leadtimes"]

    if len(R.shape) < 3:
        raise ValueError("The number of dimension must be > 2")
    if len(R.shape) == 3:
        axis = 0
    if len(R.shape) == 4:
        axis = 1
    if len(R.shape) > 4:
        raise ValueError("The number of dimension must be <= 4")

    if R.shape[axis] != len(timestamps):
        raise ValueError(
            "The list of timestamps has length %i, " % len(timestamps) + "but R contains %i frames" % R.shape[axis]
        )

    # assumes that frames are evenly spaced
    delta = (timestamps[1] - timestamps[0]).seconds / 60
    if delta == time_window_min:
        return _returned(R), metadata
    if (R.shape[axis] * delta) % time_window_min:
        raise ValueError("time_window_size does not equally split R")

    nframes = int(time_window_min / delta)

    if unit == "mm/h":
        method = "mean"
    elif unit == "mm":
        method = "sum"
    else:
        raise ValueError("can only aggregate units of 'mm/h' or 'mm'" + " not %s" % unit)
    if ignore_nan:
        method = "".join(("nan", method))

    R = aggregate_fields(R, nframes, axis=axis, method=method)

    metadata["accutime"] = time_window_min
    metadata["timestamps"] = timestamps[nframes - 1:: nframes]
    if "leadtimes" in metadata:
        metadata["leadtimes"] = leadtimes[nframes - 1:: nframes]

    return R, metadata


def _upscale_dev(R, axes, nframes, method, route="auto"):
    """Both passes of the upscale in one call: the checks the reference's two ``aggregate_fields`` calls make, in their
    order, then ``psh_aggregate_space_dev``."""
    shape = R.shape
    _check_window(shape, axes[0], nframes[0], False)
    _resident_real("aggregate_fields_space", R)
    _refuse_pairwise(shape, axes[0], nframes[0])
    mid = shape[:axes[0]] + (shape[axes[0]] // nframes[0],) + shape[axes[0] + 1:]
    _check_window(mid, axes[1], nframes[1], False)
    _refuse_pairwise(mid, axes[1], nframes[1])
    out = DeviceArray(mid[:axes[1]] + (mid[axes[1]] // nframes[1],), R.dtype)
    planes = int(np.prod(shape[:axes[0]], dtype=np.int64))
    _lib.check(_lib.lib().psh_aggregate_space_dev(R.ptr, int(R.dtype == np.float64), planes, shape[axes[0]], shape[axes[1]], nframes[0],
                                                  nframes[1], int(method == "nanmean"), _ROUTES[route], out.ptr),
               "psh_aggregate_space_dev")
    out._keep = (R, R._keep)
    return out


def aggregate_fields_space(R, metadata, space_window, ignore_nan=False):
    """Upscale fields in space; parameters, return value and metadata updates of the reference (dimension.py:120-216).
    A resident field is read once: the y pass, its rounding and the x pass run in one kernel for windows up to 64 x 64."""
    R = _own(R)
    metadata = metadata.copy()

    if space_window is None:
        return _returned(R), metadata

    unit = metadata["unit"]
    ypixelsize = metadata["ypixelsize"]
    xpixelsize = metadata["xpixelsize"]

    if len(R.shape) < 2:
        raise ValueError("The number of dimensions must be >= 2")
    if len(R.shape) == 2:
        axes = [0, 1]
    if len(R.shape) == 3:
        axes = [1, 2]
    if len(R.shape) == 4:
        axes = [2, 3]
    if len(R.shape) > 4:
        raise ValueError("The number of dimensions must be <= 4")

    if np.isscalar(space_window):
        space_window = (space_window, space_window)

    # assumes that frames are evenly spaced
    if ypixelsize == space_window[1] and xpixelsize == space_window[0]:
        return _returned(R), metadata

    ysize = R.shape[axes[0]] * ypixelsize
    xsize = R.shape[axes[1]] * xpixelsize

    if (
        abs(ysize / space_window[1] - round(ysize / space_window[1])) > 1e-10
        or abs(xsize / space_window[0] - round(xsize / space_window[0])) > 1e-10
    ):
        raise ValueError("space_window does not equally split R")

    nframes = [int(space_window[1] / ypixelsize), int(space_window[0] / xpixelsize)]

    if unit == "mm/h" or unit == "mm":
        method = "mean"
    else:
        raise ValueError("can only aggregate units of 'mm/h' or 'mm' " + "not %s" % unit)
    if ignore_nan:
        method = "".join(("nan", method))

    if isinstance(R, DeviceArray):
        R = _upscale_dev(R, axes, nframes, method)
    else:
        R = aggregate_fields(R, nframes[0], axis=axes[0], method=method)
        R = aggregate_fields(R, nframes[1], axis=axes[1], method=method)

    metadata["ypixelsize"] = space_window[1]
    metadata["xpixelsize"] = space_window[0]

    return R, metadata


def _window_dev(R, out_plane, src, dst, size, fill, dtype):
    """``out = fill; out[..., dst + size] = R[..., src + size]`` for R of shape (l, t, m, n) -> (l, t) + out_plane."""
    _resident_real("clip_domain / square_domain", R)
    out = DeviceArray(R.shape[:2] + tuple(out_plane), dtype)
    if out.dtype not in _NATIVE:
        raise NotImplementedError("clip_domain / square_domain on the device: dtype float32 or float64, not %s" % out.dtype)
    _lib.check(_lib.lib().psh_window_copy_dev(R.ptr, int(R.dtype == np.float64), R.shape[0] * R.shape[1], R.shape[2], R.shape[3], src[0],
                                              src[1], out.ptr, int(out.dtype == np.float64), out_plane[0], out_plane[1], dst[0], dst[1],
                                              size[0], size[1], float(fill)), "psh_window_copy_dev")
    out._keep = (R, R._keep)
    return out


def _as_4d(R):
    if len(R.shape) == 2:
        return _reshaped(R, (1, 1) + R.shape) if isinstance(R, DeviceArray) else R[None, None, :, :]
    if len(R.shape) == 3:
        return _reshaped(R, (1,) + R.shape) if isinstance(R, DeviceArray) else R[None, :, :, :]
    return R


def _final(R_, R_shape):
    R_shape[-2] = R_.shape[-2]
    R_shape[-1] = R_.shape[-1]
    return _reshaped(R_, tuple(int(s) for s in R_shape)) if isinstance(R_, DeviceArray) else R_.reshape(R_shape)


def _min_dev(R):
    _resident_real("square_domain", R)
    low = ctypes.c_double()
    _lib.check(_lib.lib().psh_field_min_dev(R.ptr, int(R.dtype == np.float64), R.size, ctypes.byref(low)), "psh_field_min_dev")
    return low.value


def clip_domain(R, metadata, extent=None, dtype=None):
    """Clip the field domain by geographical coordinates; parameters, return value and metadata updates of the reference
    (dimension.py:342-451).  ``dtype``: type of the result (the reference's float64 when None)."""
    resident = isinstance(R, DeviceArray)
    R = _own(R)
    R_shape = np.array(R.shape)
    metadata = metadata.copy()

    if extent is None:
        return _returned(R), metadata

    if len(R.shape) < 2:
        raise ValueError("The number of dimension must be > 1")
    if len(R.shape) > 4:
        raise ValueError("The number of dimension must be <= 4")
    R = _as_4d(R)

    # original domain and bounding box
    left, right, bottom, top = metadata["x1"], metadata["x2"], metadata["y1"], metadata["y2"]
    left_, right_, bottom_, top_ = extent[0], extent[1], extent[2], extent[3]
    xpixelsize, ypixelsize = metadata["xpixelsize"], metadata["ypixelsize"]

    # extent of the box in pixels
    dim_x_ = int((right_ - left_) / xpixelsize)
    dim_y_ = int((top_ - bottom_) / ypixelsize)
    zerovalue = metadata["zerovalue"]

    # pixel centres of the original and of the new domain
    y_coord = np.linspace(bottom, top - ypixelsize, R.shape[2]) + ypixelsize / 2.0
    x_coord = np.linspace(left, right - xpixelsize, R.shape[3]) + xpixelsize / 2.0
    y_coord_ = np.linspace(bottom_, top_ - ypixelsize, dim_y_) + ypixelsize / 2.0
    x_coord_ = np.linspace(left_, right_ - xpixelsize, dim_x_) + xpixelsize / 2.0

    # origin='upper' reverses the vertical axes direction
    if metadata["yorigin"] == "upper":
        y_coord = y_coord[::-1]
        y_coord_ = y_coord_[::-1]

    # the part of the original domain inside the box, and of the box inside the original domain
    idx_y = np.where(np.logical_and(y_coord < top_, y_coord > bottom_))[0]
    idx_x = np.where(np.logical_and(x_coord < right_, x_coord > left_))[0]
    idx_y_ = np.where(np.logical_and(y_coord_ < top, y_coord_ > bottom))[0]
    idx_x_ = np.where(np.logical_and(x_coord_ < right, x_coord_ > left))[0]

    src = (int(idx_y[0]), int(idx_x[0]))
    size = (int(idx_y[-1]) + 1 - src[0], int(idx_x[-1]) + 1 - src[1])
    dst = (int(idx_y_[0]), int(idx_x_[0]))
    size_ = (int(idx_y_[-1]) + 1 - dst[0], int(idx_x_[-1]) + 1 - dst[1])

    if resident:
        if size != size_:
            raise ValueError("could not broadcast input array from shape %s into shape %s"
                             % (str(R.shape[:2] + size).replace(" ", ""), str(R.shape[:2] + size_).replace(" ", "")))
        R_ = _window_dev(R, (dim_y_, dim_x_), src, dst, size, zerovalue, np.float64 if dtype is None else dtype)
    else:
        R_ = np.ones((R.shape[0], R.shape[1], dim_y_, dim_x_)) * zerovalue
        R_[:, :, dst[0]: dst[0] + size_[0], dst[1]: dst[1] + size_[1]] = R[:, :, src[0]: src[0] + size[0], src[1]: src[1] + size[1]]
        if dtype is not None:
            R_ = R_.astype(dtype)

    metadata["y1"] = bottom_
    metadata["y2"] = top_
    metadata["x1"] = left_
    metadata["x2"] = right_

    return _final(R_, R_shape), metadata


def _place(R, plane, at, fill, dtype):
    """A plane of ``fill`` (float64, or ``dtype``) with R (l, t, m, n) at rows / columns ``at``."""
    if isinstance(R, DeviceArray):
        return _window_dev(R, plane, (0, 0), at, R.shape[2:], fill, np.float64 if dtype is None else dtype)
    R_ = np.ones((R.shape[0], R.shape[1]) + tuple(plane)) * fill
    R_[:, :, at[0]: at[0] + R.shape[2], at[1]: at[1] + R.shape[3]] = R
    return R_ if dtype is None else R_.astype(dtype)


def _cut(R, at, size, dtype):
    """``R[:, :, rows, columns]`` in R's dtype (or ``dtype``)."""
    if isinstance(R, DeviceArray):
        return _window_dev(R, size, at, (0, 0), size, 0.0, R.dtype if dtype is None else dtype)
    R_ = R[:, :, at[0]: at[0] + size[0], at[1]: at[1] + size[1]]
    return R_ if dtype is None else R_.astype(dtype)


def square_domain(R, metadata, method="pad", inverse=False, dtype=None):
    """Pad or crop a field to a square domain, or undo that; parameters, return value and metadata updates of the reference
    (dimension.py:454-599), including two of its habits: an already square field comes back squeezed and ALONE (no
    metadata), and the inverse takes ``square_method`` / ``orig_domain`` out of the metadata it returns.  ``dtype``: type
    of the result (None: float64 where the reference builds the result with np.ones / np.zeros - a pad, the inverse of a
    crop - and the field's dtype where it slices)."""
    R = _own(R)
    R_shape = np.array(R.shape)
    metadata = metadata.copy()

    if not inverse:
        if len(R.shape) < 2:
            raise ValueError("The number of dimension must be > 1")
        if len(R.shape) > 4:
            raise ValueError("The number of dimension must be <= 4")
        R = _as_4d(R)

        if R.shape[2] == R.shape[3]:
            return _squeezed(_returned(R))

        orig_dim_y, orig_dim_x = int(R.shape[2]), int(R.shape[3])

        if method == "pad":
            new_dim = max(orig_dim_y, orig_dim_x)
            low = _min_dev(R) if isinstance(R, DeviceArray) else R.min()
            if orig_dim_x < new_dim:
                idx_buffer = int((new_dim - orig_dim_x) / 2.0)
                R_ = _place(R, (new_dim, new_dim), (0, idx_buffer), low, dtype)
                metadata["x1"] -= idx_buffer * metadata["xpixelsize"]
                metadata["x2"] += idx_buffer * metadata["xpixelsize"]
            elif orig_dim_y < new_dim:
                idx_buffer = int((new_dim - orig_dim_y) / 2.0)
                R_ = _place(R, (new_dim, new_dim), (idx_buffer, 0), low, dtype)
                metadata["y1"] -= idx_buffer * metadata["ypixelsize"]
                metadata["y2"] += idx_buffer * metadata["ypixelsize"]

        elif method == "crop":
            new_dim = min(orig_dim_y, orig_dim_x)
            if orig_dim_x > new_dim:
                idx_buffer = int((orig_dim_x - new_dim) / 2.0)
                R_ = _cut(R, (0, idx_buffer), (new_dim, new_dim), dtype)
                metadata["x1"] += idx_buffer * metadata["xpixelsize"]
                metadata["x2"] -= idx_buffer * metadata["xpixelsize"]
            elif orig_dim_y > new_dim:
                idx_buffer = int((orig_dim_y - new_dim) / 2.0)
                R_ = _cut(R, (idx_buffer, 0), (new_dim, new_dim), dtype)
                metadata["y1"] += idx_buffer * metadata["ypixelsize"]
                metadata["y2"] -= idx_buffer * metadata["ypixelsize"]

        else:
            raise ValueError("Unknown type")

        metadata["orig_domain"] = (orig_dim_y, orig_dim_x)
        metadata["square_method"] = method

        return _final(R_, R_shape), metadata

    if len(R.shape) < 2:
        raise ValueError("The number of dimension must be > 2")
    if len(R.shape) > 4:
        raise ValueError("The number of dimension must be <= 4")
    R = _as_4d(R)

    method = metadata.pop("square_method")
    shape = metadata.pop("orig_domain")
    shape = (int(shape[0]), int(shape[1]))

    if R.shape[2] == shape[0] and R.shape[3] == shape[1]:
        return _squeezed(_returned(R)), metadata

    R_ = None
    if method == "pad":
        if R.shape[2] == shape[0]:
            idx_buffer = int((R.shape[3] - shape[1]) / 2.0)
            R_ = _cut(R, (0, idx_buffer), shape, dtype)
            metadata["x1"] += idx_buffer * metadata["xpixelsize"]
            metadata["x2"] -= idx_buffer * metadata["xpixelsize"]
        elif R.shape[3] == shape[1]:
            idx_buffer = int((R.shape[2] - shape[0]) / 2.0)
            R_ = _cut(R, (idx_buffer, 0), shape, dtype)
            metadata["y1"] += idx_buffer * metadata["ypixelsize"]
            metadata["y2"] -= idx_buffer * metadata["ypixelsize"]

    elif method == "crop":
        if R.shape[2] == shape[0]:
            idx_buffer = int((shape[1] - R.shape[3]) / 2.0)
            R_ = _place(R, shape, (0, idx_buffer), 0.0, dtype)
            metadata["x1"] -= idx_buffer * metadata["xpixelsize"]
            metadata["x2"] += idx_buffer * metadata["xpixelsize"]
        elif R.shape[3] == shape[1]:
            idx_buffer = int((shape[0] - R.shape[2]) / 2.0)
            R_ = _place(R, shape, (idx_buffer, 0), 0.0, dtype)
            metadata["y1"] -= idx_buffer * metadata["ypixelsize"]
            metadata["y2"] += idx_buffer * metadata["ypixelsize"]

    if R_ is None:  # no side matches (or an unknown method): the reference's plane of zeros
        if isinstance(R, DeviceArray):
            R_ = _window_dev(R, shape, (0, 0), (0, 0), (0, 0), 0.0, np.float64 if dtype is None else dtype)
        else:
            R_ = np.zeros((R.shape[0], R.shape[1], shape[0], shape[1]), dtype=np.float64 if dtype is None else dtype)

    return _final(R_, R_shape), metadata


class TimeAggregator:
    """Running ``aggregate_fields_time`` over the lead times of a nowcast, usable as its ``callback``::

        hourly = TimeAggregator(12, method="sum", then=EnsembleProducts([10.0]))
        nowcasts.get_method("steps")(..., callback=hourly, return_output=False)
        hourly.then.excprob      # P(more than 10 mm in each hour), no member left the device

    Every call takes the members of one lead time, ``(k, m, n)`` or one field ``(m, n)``, as a ``DeviceArray`` or an
    ``ndarray``.  After every ``nframes`` calls a window closes: the aggregated block (same shape) is appended to
    ``fields`` and handed to ``then`` - as a ``DeviceArray`` if ``then.accepts_device`` and the members were resident,
    else as an ``ndarray``.  ``method``: "sum", "mean", "nansum" or "nanmean", as :func:`aggregate_fields`.

    The frames are added as they arrive, in the order NumPy adds them, so a block equals
    ``aggregate_fields(stack, nframes, axis=0, method=method)`` of the stacked frames of its window bit for bit.  float32
    members are widened and added in float64 by default - the block a nowcast returns is the float32 members widened, so
    this is the aggregate of what the reference's nowcast returns; ``dtype=np.float32`` adds in float32 and equals the
    aggregate of the float32 stack.  Frames of an incomplete last window are dropped; ``pending`` counts them.  The member
    stack is only read during the call.

    ``keep="host"`` queues one copy per block into pinned memory and waits when ``fields`` is read; ``keep="device"`` keeps
    ``DeviceArray`` blocks.  Blocks of ``ndarray`` members are computed with NumPy and kept as they are.
    """

    accepts_device = True

    def __init__(self, nframes, method="mean", then=None, keep="host", dtype=None):
        if keep not in ("host", "device"):
            raise ValueError("keep must be 'host' or 'device', not %r" % (keep,))
        if method not in _aggregation_methods:
            raise ValueError(
                "Aggregation method not recognized. " f"Available methods: {str(list(_aggregation_methods.keys()))}"
            )
        if int(nframes) <= 0:
            raise ValueError("'window_size' must be strictly positive")
        self.nframes = int(nframes)
        self.method = method
        self.then = then
        self.keep = keep
        self.dtype = None if dtype is None else np.dtype(dtype)
        if self.dtype is not None and self.dtype not in _NATIVE:
            raise NotImplementedError("TimeAggregator: dtype float32 or float64, not %s" % self.dtype)
        self.pending = 0  # frames of the window that is open
        self.received = []  # type of the members of every call: DeviceArray or ndarray
        self._fields = []
        self._copies_queued = False
        self._acc = None
        self._count = None

    def _acc_dtype(self, members_dtype):
        if members_dtype not in _NATIVE:
            raise NotImplementedError("TimeAggregator: float32 or float64 members, not %s" % members_dtype)
        want = np.dtype(np.float64) if self.dtype is None else self.dtype
        if want == np.float32 and members_dtype == np.float64:
            raise ValueError("TimeAggregator: float64 members cannot be accumulated in float32")
        return want

    def __call__(self, members):
        resident = isinstance(members, DeviceArray)
        self.received.append(DeviceArray if resident else np.ndarray)
        if not resident:
            members = np.asarray(members)
        if len(members.shape) not in (2, 3):
            raise ValueError("TimeAggregator: members of shape (k, m, n) or (m, n) expected, got %s" % (tuple(members.shape),))
        dtype = self._acc_dtype(members.dtype)
        first, last = self.pending == 0, self.pending == self.nframes - 1
        if not first and (tuple(self._acc.shape) != tuple(members.shape) or isinstance(self._acc, DeviceArray) != resident):
            raise ValueError("TimeAggregator: the members changed within a window (%s after %s)"
                             % (tuple(members.shape), tuple(self._acc.shape)))
        if resident:
            self._step_dev(members, dtype, first, last)
        else:
            self._step_host(members, dtype, first, last)
        self.pending += 1
        if last:
            self._close(resident)

    def _step_dev(self, members, dtype, first, last):
        if first:
            self._acc = DeviceArray(members.shape, dtype)
            if self.method == "nanmean" and (self._count is None or self._count.shape != members.shape):
                self._count = DeviceArray(members.shape, np.uint32)
        count = self._count.ptr if self.method == "nanmean" else None
        _lib.check(_lib.lib().psh_accumulate_step_dev(members.ptr, int(members.dtype == np.float64), self._acc.ptr,
                                                      int(dtype == np.float64), count, members.size, _METHOD_CODES[self.method],
                                                      int(first), int(last), self.nframes), "psh_accumulate_step_dev")

    def _step_host(self, members, dtype, first, last):
        skip = self.method in ("nansum", "nanmean")
        frame = members.astype(dtype)
        valid = ~np.isnan(frame)
        if skip:
            frame[~valid] = 0
        if first:
            self._acc, self._count = frame + dtype.type(0), valid.astype(np.intp)  # NumPy's sums start from +0
        else:
            self._acc = self._acc + frame
            self._count = self._count + valid
        if last and self.method in ("mean", "nanmean"):
            with np.errstate(invalid="ignore", divide="ignore"):
                div = np.intp(self.nframes) if self.method == "mean" else self._count
                self._acc = np.true_divide(self._acc, div, out=self._acc, casting="unsafe")

    def _close(self, resident):
        block, self._acc, self.pending = self._acc, None, 0
        then_block = block
        if resident:
            if self.then is not None and not getattr(self.then, "accepts_device", False):
                then_block = block.to_host()
            if self.keep == "host":
                if then_block is not block:
                    block = then_block
                else:
                    from .. import _pinned  # noqa: PLC0415

                    host = _pinned.empty(block.shape, block.dtype)
                    _lib.check(_lib.lib().psh_memcpy_d2h_async(host.ctypes.data, block.ptr, block.nbytes), "psh_memcpy_d2h_async")
                    self._copies_queued = True
                    block = host
        self._fields.append(block)
        if self.then is not None:
            self.then(then_block)

    @property
    def fields(self):
        """The aggregated blocks, one per closed window."""
        if self._copies_queued:
            _lib.check(_lib.lib().psh_sync(), "psh_sync")
            self._copies_queued = False
        return self._fields

    @property
    def n_windows(self):
        return len(self._fields)
