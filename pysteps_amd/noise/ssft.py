"""Short-space Fourier (ssft / nested) noise on the GPU: mirrors of pysteps/noise/fftgenerators.py:442-852
(``initialize_nonparam_2d_ssft_filter``, ``initialize_nonparam_2d_nested_filter``, ``generate_noise_2d_ssft_filter``).

The reference's local filters are real full-spectrum planes ``F[i, j]`` and its generator forms
``Re(ifft2(fft2(N) * F[i, j]))`` per window with ``N`` real.  ``fft2(N)`` is Hermitian, so that real part is ``irfft2`` of
the ``rfft2`` half of ``fft2(N) * Fs`` with ``Fs(k) = (F(k) + F(-k)) / 2`` - for the filters the initialisers build
``Fs == F`` up to rounding, for any other 4-D array the fold is exact in real arithmetic.  The device keeps
``(m, n//2+1)`` half planes, each DISTINCT plane once (windows that do not pass the wet-area test share the global
filter), and runs one ``rfft2`` of the white noise and one ``irfft2`` per distinct plane (csrc/ssft.hip).

What stays on the host is what is cheap, order-dependent or part of the reference's contract: the field preparation
(``rm_rdisc``, minimum subtraction), the window rectangles (the reference's own integer expressions), the mask tiles, the
sum of masks ``sM`` (it does not depend on the noise), the wet-area ratio's division and comparison, the draw of the
white noise.  The initialisers return the reference's dictionary - a host 4-D ``"field"`` expanded from the half planes
by symmetry - or, with ``resident=True``, a :class:`FilterBank` that never leaves the device; the generator takes both.
Calls the device does not take run the reference's function with a ``RuntimeWarning`` that says why.
"""

import hashlib
import warnings
import weakref

import numpy as np

from .. import _lib
from .._reference import lookup
from ..cascade.decomposition import _device_nonfinite, _fingerprint
from ..device import DeviceArray
from ..utils import fft as hip_fft
from .randstate import DeviceRandomStates

__all__ = ["initialize_nonparam_2d_ssft_filter", "initialize_nonparam_2d_nested_filter", "generate_noise_2d_ssft_filter",
           "generate_noise_table", "FilterBank"]

# device memory the half planes of one filter bank may take; a bank beyond it is left to the reference
BANK_BYTES = 8 << 30

_NONFINITE_FILTER = (
    "field contains non-finite values, this typically happens when the input\n"
    + "precipitation field provided to pysteps contains (mostly) zero value.s\n"
    + "To prevent this error please call pysteps.utils.check_norain first,\n"
    + "using the same win_fun as used in this method (tukey by default)\n"
    + "and then only call this method if that check fails."
)


# ---- geometry and masks: host, the reference's arithmetic ------------------------------------------------------------
def window_function(m, n, func):
    """The tapering weights of pysteps/utils/tapering.py ``compute_window_function(m, n, func)`` ('hann' or 'tukey'
    with alpha 0.2): a function of the distance from the centre of the region, operation by operation."""
    x = np.arange(n) / n - 0.5
    y = np.arange(m) / m - 0.5
    R = np.sqrt(x[None, :] ** 2 + y[:, None] ** 2)
    W = np.ones_like(R)
    if func == "hann":
        inside = ~(R > 0.5)
        W[~inside] = 0.0
        W[inside] = 0.5 * (1.0 - np.cos(2.0 * np.pi * (R[inside] + 0.5)))
    elif func == "tukey":
        alpha = 0.2
        band = np.logical_and(R < 0.5, R > 0.5 * (1.0 - alpha))
        W[band] = 0.5 * (1.0 + np.cos(np.pi * (R[band] / (alpha * 0.5) - 1.0 / alpha + 1.0)))
        W[R >= 0.5] = 0.0
    else:
        raise ValueError("invalid window function '%s'" % func)
    return W


def mask_tile(height, width, win_fun):
    """The window of ``_get_mask`` (fftgenerators.py:882-899) without the zeros around it: the tapering weights plus
    1e-6, or None for ``win_fun=None`` (a mask of ones)."""
    if win_fun is None:
        return None
    return window_function(height, width, win_fun) + 1e-6


def ssft_rectangles(dim, win_size, overlap, ny, nx):
    """``(ny * nx, 4)`` int64 rows ``[i0, i1, j0, j1]`` of the windows of fftgenerators.py:544-555 / :825-841, row-major."""
    dim_y, dim_x = dim
    rects = np.empty((ny * nx, 4), dtype=np.int64)
    for i in range(ny):
        for j in range(nx):
            i0 = int(np.max((i * win_size[0] - overlap * win_size[0], 0)))
            i1 = int(np.min((i0 + win_size[0] + overlap * win_size[0], dim_y)))
            j0 = int(np.max((j * win_size[1] - overlap * win_size[1], 0)))
            j1 = int(np.min((j0 + win_size[1] + overlap * win_size[1], dim_x)))
            rects[i * nx + j] = (i0, i1, j0, j1)
    return rects


def split_field(idxi, idxj, segments):
    """``_split_field`` (fftgenerators.py:855-879): ``(segments**2, 2)`` int arrays of row and column bounds."""
    sizei = idxi[1] - idxi[0]
    sizej = idxj[1] - idxj[0]
    winsizei = int(sizei / segments)
    winsizej = int(sizej / segments)
    Idxi = np.zeros((segments ** 2, 2))
    Idxj = np.zeros((segments ** 2, 2))
    for i in range(segments):
        for j in range(segments):
            k = i * segments + j
            Idxi[k, 0] = idxi[0] + i * winsizei
            Idxi[k, 1] = np.min((Idxi[k, 0] + winsizei, idxi[1]))
            Idxj[k, 0] = idxj[0] + j * winsizej
            Idxj[k, 1] = np.min((Idxj[k, 0] + winsizej, idxj[1]))
    return Idxi.astype(int), Idxj.astype(int)


def nested_levels(dim, max_level):
    """Per level of the nested initialiser (fftgenerators.py:674-730) the list of ``(rectangle, cell block)`` pairs in
    the reference's loop order: ``rectangle = (i0, i1, j0, j1)`` of the field, ``cell block = (a0, a1, b0, b1)`` of the
    ``2**max_level`` square grid of filters."""
    side = 2 ** max_level
    Idxi, Idxj = np.array([[0, dim[0]]]), np.array([[0, dim[1]]])
    Pi, Pj = np.array([[0, side]]), np.array([[0, side]])
    levels = []
    for level in range(max_level):
        entries = []
        for k in range(len(Idxi)):
            ni, nj = split_field(Idxi[k, :], Idxj[k, :], 2)
            pi, pj = split_field(Pi[k, :], Pj[k, :], 2)
            for q in range(len(ni)):
                entries.append(((int(ni[q, 0]), int(ni[q, 1]), int(nj[q, 0]), int(nj[q, 1])),
                                (int(pi[q, 0]), int(pi[q, 1]), int(pj[q, 0]), int(pj[q, 1]))))
        levels.append(entries)
        Idxi, Idxj = split_field((0, dim[0]), (0, dim[1]), 2 ** (level + 1))
        Pi, Pj = split_field((0, side), (0, side), 2 ** (level + 1))
    return levels


def merge_weights(dim, gridres, height):
    """The logistic weights of fftgenerators.py:704-710 for a window of ``height`` rows, on the ``rfft2`` half plane.
    The DC bin (``freq_grid == 0``) takes what NumPy gives it: 1 / 0 = inf, exp(-inf) = 0, weight 1."""
    fx, fy = np.meshgrid(np.fft.fftfreq(dim[1], gridres), np.fft.fftfreq(dim[0], gridres))
    freq_grid = np.sqrt(fx ** 2 + fy ** 2)
    k = 0.05
    x0 = height / 2.0
    with np.errstate(divide="ignore"):
        weights = 1 / (1 + np.exp(-k * (1 / freq_grid - x0 * gridres)))
    return np.ascontiguousarray(weights[:, : dim[1] // 2 + 1])


def prepare_field(field, rm_rdisc):
    """fftgenerators.py:508-523: a float copy ``(nr_fields, m, n)`` with the rain / no-rain discontinuity removed and
    every field's minimum at zero."""
    field = field.copy()
    if rm_rdisc:
        field[field > field.min()] -= field[field > field.min()].min() - field.min()
    if len(field.shape) == 2:
        field = field[None, :, :]
    field -= field.min(axis=(1, 2))[:, None, None]
    return field


def fold_half(F):
    """``(F(k) + F(-k)) / 2`` on the ``rfft2`` half plane, for the last two axes of a real full-spectrum array."""
    n = F.shape[-1]
    mirrored = np.roll(np.flip(F, axis=(-2, -1)), (1, 1), axis=(-2, -1))
    return np.ascontiguousarray(((F + mirrored) / 2)[..., : n // 2 + 1])


def expand_half(half, n):
    """The full-spectrum plane(s) ``(..., m, n)`` of half planes ``(..., m, n//2+1)`` that are symmetric under k -> -k."""
    nc = half.shape[-1]
    full = np.empty(half.shape[:-1] + (n,), dtype=half.dtype)
    full[..., :nc] = half
    if n > nc:
        mirrored = np.roll(np.flip(half, axis=-2), 1, axis=-2)  # rows -k
        full[..., nc:] = mirrored[..., n - nc : 0 : -1]
    return full


class _Tiles:
    """Mask tiles by shape, each once, laid out one after the other for the device."""

    def __init__(self, win_fun):
        self.win_fun = win_fun
        self.offsets = {}
        self.tiles = {}
        self.count = 0

    def offset(self, height, width):
        if self.win_fun is None:
            return -1
        key = (int(height), int(width))
        if key not in self.offsets:
            self.offsets[key] = self.count
            self.tiles[key] = mask_tile(key[0], key[1], self.win_fun)
            self.count += key[0] * key[1]
        return self.offsets[key]

    def tile(self, height, width):
        return None if self.win_fun is None else self.tiles[(int(height), int(width))]

    def upload(self):
        if not self.count:
            return None
        return DeviceArray.from_host(np.concatenate([t.ravel() for t in self.tiles.values()]))


def _table(rects, tiles, planes):
    """The (nwin, 6) int64 window table of csrc/ssft.hip: rectangle, tile offset, plane."""
    table = np.empty((len(rects), 6), dtype=np.int64)
    for k, (i0, i1, j0, j1) in enumerate(rects):
        table[k] = (i0, i1, j0, j1, tiles.offset(i1 - i0, j1 - j0), planes[k])
    return table


class _Plan:
    """What the generator needs beside the planes for one ``(overlap, win_fun)``: rectangles, mask tiles, ``sM``."""

    def __init__(self, bank, overlap, win_fun):
        ny, nx, m, n = bank.shape
        win_size = (float(m) / ny, float(n) / nx)  # fftgenerators.py:820
        self.rects = ssft_rectangles((m, n), win_size, overlap, ny, nx)
        tiles = _Tiles(win_fun)
        self.table = _table(self.rects, tiles, bank.plane_of.ravel())
        sM = np.zeros((m, n))
        for i0, i1, j0, j1 in self.rects:  # sM += M window by window; outside the rectangle M adds zero
            tile = tiles.tile(i1 - i0, j1 - j0)
            sM[i0:i1, j0:j1] += 1.0 if tile is None else tile
        self.sM_host = sM
        self.sM = DeviceArray.from_host(sM)
        self.tiles = tiles.upload()
        self.tiles_count = tiles.count


class FilterBank:
    """A filter bank on the device: the distinct half planes ``(nplanes, m, n//2+1)``, the window-to-plane map
    ``plane_of (ny, nx)`` and, per ``(overlap, win_fun)`` the generator is called with, the cached rectangles, mask
    tiles and sum of masks.  ``shape`` is that of the reference's 4-D array, ``(ny, nx, m, n)``."""

    def __init__(self, planes, plane_of, input_shape, war_counts=None):
        m, n = (int(s) for s in input_shape)
        self.planes = planes
        self.plane_of = np.ascontiguousarray(plane_of, dtype=np.int64)
        self.shape = tuple(int(s) for s in self.plane_of.shape) + (m, n)
        self.dtype = np.dtype(np.float64)
        self.war_counts = war_counts
        self._plans = {}
        self._finite = None

    @property
    def nplanes(self):
        return int(self.planes.shape[0])

    def plan(self, overlap, win_fun):
        key = (float(overlap), win_fun)
        if key not in self._plans:
            self._plans[key] = _Plan(self, overlap, win_fun)
        return self._plans[key]

    def all_finite(self):
        if self._finite is None:
            self._finite = not _device_nonfinite(self.planes)
        return self._finite

    def half_planes(self):
        """The distinct half planes on the host, ``(nplanes, m, n//2+1)``."""
        return self.planes.to_host()

    def to_full(self):
        """The reference's 4-D array ``(ny, nx, m, n)``, expanded from the half planes by symmetry."""
        full = expand_half(np.asarray(self.half_planes()), self.shape[3])
        return full[self.plane_of]


# ---- declined calls -------------------------------------------------------------------------------------------------
def _to_reference(name, ours, reason, args, kwargs):
    ref = lookup("noise.fftgenerators", name, ours)
    if ref is None:
        raise NotImplementedError("pysteps_amd %s: %s, and pysteps is not importable for the reference's function" % (name, reason))
    warnings.warn("pysteps_amd %s: %s - running the reference's function" % (name, reason), RuntimeWarning, stacklevel=3)
    return ref(*args, **kwargs)


def _init_decline_reason(field):
    if not isinstance(field, np.ndarray):
        return "the input is not a NumPy array"
    if field.dtype != np.float64:
        return "the input is %s, the device path is float64" % field.dtype
    shape = tuple(int(s) for s in field.shape[-2:])
    if not hip_fft.supported_shape(shape):
        return "the HIP transforms do not take the shape %s" % (shape,)
    if shape[0] * (shape[1] // 2 + 1) * 8 > BANK_BYTES:
        return "a filter plane does not fit the memory budget of %d bytes" % BANK_BYTES
    return None


def _check_init_input(field):
    if len(field.shape) < 2 or len(field.shape) > 3:
        raise ValueError("the input is not two- or three-dimensional array")
    if np.any(np.isnan(field)):
        raise ValueError("field must not contain NaNs")


# ---- the initialisers ------------------------------------------------------------------------------------------------
class _Builder:
    """The device side of one initialiser call: the prepared stack, wet-area counts and local filters."""

    def __init__(self, fields):
        self.lib = _lib.lib()
        self.nr_fields, self.m, self.n = (int(s) for s in fields.shape)
        self.nc = self.n // 2 + 1
        self.fields = DeviceArray.from_host(np.ascontiguousarray(fields, dtype=np.float64))

    def war_counts(self, rects, win_fun):
        """The integer counts of ``field * mask > 0.01`` of every window, one launch."""
        tiles = _Tiles(win_fun)
        table = _table(rects, tiles, [0] * len(rects))
        d_tiles = tiles.upload()
        counts = DeviceArray((len(rects),), np.uint64)
        _lib.check(self.lib.psh_ssft_war_counts_dev(self.fields.ptr, self.nr_fields, self.m, self.n, table.ctypes.data, len(rects),
                                                    d_tiles.ptr if d_tiles is not None else None, tiles.count, counts.ptr),
                   "psh_ssft_war_counts_dev")
        return counts.to_host().astype(np.int64), (tiles, d_tiles)

    def filters(self, rects, tiles, d_tiles, plane_indices, planes, taper_after=False):
        """The local filters of ``rects`` into the planes ``plane_indices`` of ``planes``."""
        if not len(rects):
            return
        table = _table(rects, tiles, plane_indices)
        _lib.check(self.lib.psh_ssft_local_filters_dev(self.fields.ptr, self.nr_fields, self.m, self.n, table.ctypes.data, len(rects),
                                                       d_tiles.ptr if d_tiles is not None else None, tiles.count,
                                                       1 if taper_after else 0, int(planes.shape[0]), planes.ptr),
                   "psh_ssft_local_filters_dev")

    def global_filter(self, win_fun, planes, index=0):
        """``F0``: the whole domain as one window, the prepared field tapered by ``win_fun`` itself (no 1e-6 offset)."""
        tiles = _Tiles(None)
        d_tiles = None
        if win_fun is not None:
            tiles.win_fun = win_fun
            tiles.offsets[(self.m, self.n)] = 0
            tiles.tiles[(self.m, self.n)] = window_function(self.m, self.n, win_fun)
            tiles.count = self.m * self.n
            d_tiles = tiles.upload()
        self.filters([(0, self.m, 0, self.n)], tiles, d_tiles, [index], planes, taper_after=True)


def _result(bank, resident):
    return {"field": bank if resident else bank.to_full(), "input_shape": bank.shape[2:], "use_full_fft": True}


def initialize_nonparam_2d_ssft_filter(field, **kwargs):
    """Local Fourier filters by the short-space Fourier transform (parameters, defaults and return value as documented
    for the reference, fftgenerators.py:442-488).  ``resident=True``, the one keyword beyond the reference's: ``"field"``
    is a :class:`FilterBank` on the device instead of the host 4-D array.  ``fft_method`` is accepted and not used: the
    transforms are the device's."""
    _check_init_input(field)
    resident = bool(kwargs.get("resident", False))
    reason = _init_decline_reason(field)
    if reason is not None:
        ref_kwargs = {k: v for k, v in kwargs.items() if k != "resident"}
        return _to_reference("initialize_nonparam_2d_ssft_filter", initialize_nonparam_2d_ssft_filter, reason, (field,), ref_kwargs)

    win_size = kwargs.get("win_size", (128, 128))
    if type(win_size) == int:
        win_size = (win_size, win_size)
    win_fun = kwargs.get("win_fun", "tukey")
    overlap = kwargs.get("overlap", 0.3)
    war_thr = kwargs.get("war_thr", 0.1)
    rm_rdisc = kwargs.get("rm_rdisc", True)

    fields = prepare_field(field, rm_rdisc)
    nr_fields, dim_y, dim_x = fields.shape
    ny = int(np.ceil(float(dim_y) / win_size[0]))
    nx = int(np.ceil(float(dim_x) / win_size[1]))
    rects = ssft_rectangles((dim_y, dim_x), win_size, overlap, ny, nx)

    build = _Builder(fields)
    counts, (tiles, d_tiles) = build.war_counts(rects, win_fun)
    passed = []
    for k, (i0, i1, j0, j1) in enumerate(rects):
        war = float(counts[k]) / ((i1 - i0) * (j1 - j0) * nr_fields)  # fftgenerators.py:560-562
        if war > war_thr:
            passed.append(k)
    nplanes = 1 + len(passed)
    if nplanes * dim_y * (dim_x // 2 + 1) * 8 > BANK_BYTES:
        ref_kwargs = {k: v for k, v in kwargs.items() if k != "resident"}
        return _to_reference("initialize_nonparam_2d_ssft_filter", initialize_nonparam_2d_ssft_filter,
                             "%d filter planes do not fit the memory budget of %d bytes" % (nplanes, BANK_BYTES), (field,), ref_kwargs)
    planes = DeviceArray((nplanes, dim_y, dim_x // 2 + 1), np.float64)
    build.global_filter(win_fun, planes, 0)
    build.filters([rects[k] for k in passed], tiles, d_tiles, list(range(1, nplanes)), planes)
    plane_of = np.zeros(ny * nx, dtype=np.int64)
    plane_of[passed] = np.arange(1, nplanes)
    bank = FilterBank(planes, plane_of.reshape(ny, nx), (dim_y, dim_x), war_counts=counts.reshape(ny, nx))
    return _result(bank, resident)


def initialize_nonparam_2d_nested_filter(field, gridres=1.0, **kwargs):
    """Local Fourier filters by the nested approach (parameters, defaults and return value as documented for the
    reference, fftgenerators.py:577-618).  ``resident=True``: ``"field"`` is a :class:`FilterBank` on the device."""
    _check_init_input(field)
    resident = bool(kwargs.get("resident", False))
    reason = _init_decline_reason(field)
    max_level = kwargs.get("max_level", 3)
    if reason is None and (4 ** max_level + 1) * field.shape[-2] * (field.shape[-1] // 2 + 1) * 8 > BANK_BYTES:
        reason = "%d filter planes do not fit the memory budget of %d bytes" % (4 ** max_level, BANK_BYTES)
    if reason is not None:
        ref_kwargs = {k: v for k, v in kwargs.items() if k != "resident"}
        return _to_reference("initialize_nonparam_2d_nested_filter", initialize_nonparam_2d_nested_filter, reason, (field, gridres),
                             ref_kwargs)

    win_fun = kwargs.get("win_fun", "tukey")
    war_thr = kwargs.get("war_thr", 0.1)
    rm_rdisc = kwargs.get("rm_rdisc", True)

    fields = prepare_field(field, rm_rdisc)
    nr_fields, dim_y, dim_x = fields.shape
    half = dim_y * (dim_x // 2 + 1)
    side = 2 ** max_level
    lib = _lib.lib()
    build = _Builder(fields)

    # the planes in use, each a (1, m, n//2+1) DeviceArray; cells of the side x side grid share a plane until a merge
    # reaches one of them and not the other (copy on write)
    planes = [DeviceArray((1, dim_y, dim_x // 2 + 1), np.float64)]
    build.global_filter(win_fun, planes[0], 0)
    plane_of = np.zeros((side, side), dtype=np.int64)
    fresh = DeviceArray((1, dim_y, dim_x // 2 + 1), np.float64)
    all_counts = []
    for entries in nested_levels((dim_y, dim_x), max_level):
        rects = [e[0] for e in entries]
        counts, (tiles, d_tiles) = build.war_counts(rects, win_fun)
        all_counts.append(counts)
        for k, ((i0, i1, j0, j1), (a0, a1, b0, b1)) in enumerate(entries):
            war = counts[k] / float((i1 - i0) * (j1 - j0) * nr_fields)  # fftgenerators.py:685-689
            if not war > war_thr:
                continue
            build.filters([rects[k]], tiles, d_tiles, [0], fresh)
            weights = DeviceArray.from_host(merge_weights((dim_y, dim_x), gridres, i1 - i0))
            block = np.zeros((side, side), dtype=bool)
            block[a0:a1, b0:b1] = True
            for p in np.unique(plane_of[block]):
                if np.any(plane_of[~block] == p):  # shared with cells outside the block: the block's cells get a copy
                    copy = DeviceArray((1, dim_y, dim_x // 2 + 1), np.float64)
                    _lib.check(lib.psh_memcpy_d2d(copy.ptr, planes[p].ptr, half * 8), "psh_memcpy_d2d")
                    planes.append(copy)
                    plane_of[block & (plane_of == p)] = len(planes) - 1
                    p = len(planes) - 1
                _lib.check(lib.psh_ssft_merge_dev(planes[p].ptr, weights.ptr, fresh.ptr, half), "psh_ssft_merge_dev")
    packed = DeviceArray((len(planes), dim_y, dim_x // 2 + 1), np.float64)
    for p, plane in enumerate(planes):
        _lib.check(lib.psh_memcpy_d2d(packed.ptr + p * half * 8, plane.ptr, half * 8), "psh_memcpy_d2d")
    bank = FilterBank(packed, plane_of, (dim_y, dim_x), war_counts=all_counts)
    return _result(bank, resident)


# ---- the generator ---------------------------------------------------------------------------------------------------
_bank_cache = {}  # id(host 4-D array) -> (weakref, fingerprint, FilterBank)


def _bank_of_host(F, input_shape):
    """The device bank of a host 4-D filter array: folded to half planes, identical planes kept once, uploaded once and
    cached while the array lives (and keeps its content)."""
    key = id(F)
    hit = _bank_cache.get(key)
    fp = _fingerprint(F)
    if hit is not None and hit[0]() is F and hit[1] == fp:
        return hit[2]
    ny, nx = F.shape[:2]
    seen, distinct = {}, []
    plane_of = np.empty((ny, nx), dtype=np.int64)
    for i in range(ny):
        for j in range(nx):
            plane = np.ascontiguousarray(F[i, j], dtype=np.float64)
            digest = hashlib.blake2b(plane.tobytes(), digest_size=16).digest()
            if digest not in seen:
                seen[digest] = len(distinct)
                distinct.append(fold_half(plane))
            plane_of[i, j] = seen[digest]
    bank = FilterBank(DeviceArray.from_host(np.stack(distinct)), plane_of, input_shape)
    bank._finite = True  # the caller has checked the array
    try:
        ref = weakref.ref(F, lambda _r, k=key: _bank_cache.pop(k, None))
    except TypeError:
        return bank
    _bank_cache[key] = (ref, fp, bank)
    return bank


def _generator_bank(F, kwargs):
    """The checks of fftgenerators.py:770-788 and the bank, or the reason the device declines."""
    field = F["field"]
    if len(field.shape) != 4:
        raise ValueError("the input is not four-dimensional array")
    resident = isinstance(field, FilterBank)
    if not (field.all_finite() if resident else np.all(np.isfinite(field))):
        raise ValueError(_NONFINITE_FILTER)
    if "domain" in kwargs.keys() and kwargs["domain"] == "spectral":
        raise NotImplementedError("SSFT-based noise generator is not implemented in the spectral domain")
    if resident:
        return field, None
    shape = tuple(int(s) for s in field.shape[2:])
    if field.dtype != np.float64:
        return None, "the filter is %s, the device path is float64" % field.dtype
    if not hip_fft.supported_shape(shape):
        return None, "the HIP transforms do not take the shape %s" % (shape,)
    if field.shape[0] * field.shape[1] * shape[0] * (shape[1] // 2 + 1) * 8 > BANK_BYTES:
        return None, "%d filter planes do not fit the memory budget of %d bytes" % (field.shape[0] * field.shape[1], BANK_BYTES)
    return _bank_of_host(field, shape), None


def _generate(bank, white, overlap, win_fun):
    """``white`` (K, m, n) float64 DeviceArray -> (K, m, n) DeviceArray of composites."""
    K, m, n = (int(s) for s in white.shape)
    plan = bank.plan(overlap, win_fun)
    out = DeviceArray((K, m, n), np.float64)
    _lib.check(_lib.lib().psh_ssft_generate_dev(white.ptr, K, m, n, bank.planes.ptr, bank.nplanes, plan.table.ctypes.data,
                                                len(plan.table), plan.tiles.ptr if plan.tiles is not None else None,
                                                plan.tiles_count, plan.sM.ptr, out.ptr), "psh_ssft_generate_dev")
    return out


def generate_noise_2d_ssft_filter(F, randstate=None, seed=None, **kwargs):
    """Locally correlated noise from a bank of local Fourier filters (parameters, defaults and return value as
    documented for the reference, fftgenerators.py:735-769).  ``F["field"]`` is the host 4-D array of either
    implementation's initialiser or a :class:`FilterBank`.  ``fft_method`` is accepted and not used."""
    bank, reason = _generator_bank(F, kwargs)
    if reason is not None:
        return _to_reference("generate_noise_2d_ssft_filter", generate_noise_2d_ssft_filter, reason, (F,),
                             dict(kwargs, randstate=randstate, seed=seed))
    overlap = kwargs.get("overlap", 0.2)
    win_fun = kwargs.get("win_fun", "tukey")
    if randstate is None:
        randstate = np.random
    if seed is not None:
        randstate.seed(seed)
    dim_y, dim_x = bank.shape[2:]
    N = randstate.randn(dim_y, dim_x)  # fftgenerators.py:809
    white = DeviceArray.from_host(N.reshape(1, dim_y, dim_x))
    return _generate(bank, white, overlap, win_fun).to_host().reshape(dim_y, dim_x)


def generate_noise_table(F, randstates, K, **kwargs):
    """``K`` noise fields against one filter bank in one call: ``randstates`` is a
    :class:`~pysteps_amd.noise.randstate.DeviceRandomStates` of ``K`` generators, each of which draws its
    ``randn(m, n)`` on the device; returns a float64 ``(K, m, n)`` :class:`~pysteps_amd.device.DeviceArray` whose plane
    ``k`` holds the bits of a single call with generator ``k``.  ``overlap`` and ``win_fun`` as for the generator."""
    if not isinstance(randstates, DeviceRandomStates) or randstates.n != int(K):
        raise ValueError("generate_noise_table: randstates must be a DeviceRandomStates of K generators")
    bank, reason = _generator_bank(F, kwargs)
    if reason is not None:
        raise NotImplementedError("pysteps_amd generate_noise_table: %s" % reason)
    dim_y, dim_x = bank.shape[2:]
    white = randstates.randn(dim_y, dim_x)
    return _generate(bank, white, kwargs.get("overlap", 0.2), kwargs.get("win_fun", "tukey"))
