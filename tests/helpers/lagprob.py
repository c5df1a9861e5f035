"""NumPy integer restatement of the probability stage of pysteps/nowcasts/lagrangian_probability.py (test yardstick).

The reference divides ``convolve(exceed, kernel, mode="same")`` by ``convolve(valid, kernel, mode="same")``, two 0/1
maps and a 0/1 kernel, so both are integers; SciPy's FFT path returns them with an error near 1e-7.  Here they are
counted: row prefix sums of the maps, one difference per run of ones of every kernel row.  ``mode="same"`` takes
``full[y + c, x + c]``, ``c = (scale - 1) // 2``, of the true convolution, so kernel entry ``(i, j)`` meets the input
pixel ``(y + c - i, x + c - j)``; pixels outside the image are zero.
"""

import numpy as np


def get_kernel(size):
    """The reference's kernel from its formula: ones below size 5, else the disc around ``size // 2``."""
    if size < 5:
        return np.ones((size, size), dtype=bool)
    middle = size // 2
    ii, jj = np.mgrid[:size, :size]
    return (ii - middle) ** 2 + (jj - middle) ** 2 <= middle**2


def support_of(kernel):
    """Set of (dy, dx) input offsets that ``convolve(..., kernel, mode="same")`` sums for an output pixel."""
    s = kernel.shape[0]
    c = (s - 1) // 2
    ii, jj = np.nonzero(kernel)
    return set(zip((c - ii).tolist(), (c - jj).tolist()))


def _runs(row):
    """[(first, last)] of the runs of True in a 1-d boolean array."""
    idx = np.flatnonzero(row)
    if idx.size == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) > 1)
    starts = np.concatenate([[idx[0]], idx[cut + 1]])
    ends = np.concatenate([idx[cut], [idx[-1]]])
    return list(zip(starts.tolist(), ends.tolist()))


def neighbourhood_counts(binary, kernel, rows=None):
    """``convolve(binary, kernel, mode="same")`` in integers, for the output rows ``rows`` (all by default)."""
    m, n = binary.shape
    s = kernel.shape[0]
    c = (s - 1) // 2
    rows = np.arange(m) if rows is None else np.asarray(rows)
    prefix = np.zeros((m, n + 1), dtype=np.int64)
    np.cumsum(binary, axis=1, out=prefix[:, 1:])
    xs = np.arange(n)
    out = np.zeros((rows.size, n), dtype=np.int64)
    for i in range(s):
        src = rows + c - i
        ok = (src >= 0) & (src < m)
        if not ok.any():
            continue
        lines = prefix[src[ok]]
        for j0, j1 in _runs(kernel[i]):
            right = np.clip(xs + c - j0 + 1, 0, n)
            left = np.clip(xs + c - j1, 0, n)
            out[ok] += lines[:, right] - lines[:, left]
    return out


def probability(field, threshold, scale, rows=None):
    """One lead time of the reference's probability stage on the advected ``field`` (m, n), exact: float64
    ``count(exceed) / count(valid)`` under the kernel, NaN where ``field`` is NaN; ``scale == 0`` is the 0/1 map."""
    field = np.asarray(field)
    nan = np.isnan(field)
    valid = ~nan
    exceed = np.zeros(field.shape, dtype=bool)
    exceed[valid] = field[valid].astype(np.float64) >= threshold
    sel = slice(None) if rows is None else np.asarray(rows)
    if scale == 0:
        out = exceed[sel].astype(np.float64)
    else:
        kernel = get_kernel(scale)
        ce = neighbourhood_counts(exceed, kernel, rows)
        cv = neighbourhood_counts(valid, kernel, rows)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = np.clip(ce.astype(np.float64) / cv.astype(np.float64), 0, 1)
    out[nan[sel]] = np.nan
    return out


def probability_stack(fields, threshold, scales):
    return np.stack([probability(f, threshold, int(s)) for f, s in zip(fields, scales)])
