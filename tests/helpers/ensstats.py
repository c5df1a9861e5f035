"""NumPy restatement of the three rules csrc/ensstats.hip is written to (pysteps/postprocessing/ensemblestats.py
``mean`` and ``excprob`` as explicit loops over the members, in member order).  tests/test_ensstats_cpu.py holds it to the
reference's goldens bit for bit; the GPU tests use it where no golden exists.

* mean, plain: ``s = 0; s += X[j]`` in member order in the stack's own type (``np.add.reduce`` starts from its identity
  ``+0.0``, so members that are all ``-0.0`` give ``+0.0``), then ``s / k`` in that type.
* mean, ``ignore_nan`` or ``X_thr``: values ``< X_thr`` count as NaN; NaN (not inf) adds 0 to the sum and nothing to the
  count; the sum starts from 0 in member order; ``sum / count`` in the stack's type, ``0 / 0`` = NaN.
* excprob: ``count = #{finite and >= thr}`` compared in float64, ``nfinite = #{finite}``; ``count / k`` (one float64
  division) where ``nfinite == k`` else NaN; with ``ignore_nan`` ``count / nfinite``, NaN where ``nfinite == 0``.

A threshold meets the stack as NumPy's promotion rules say (``compared_as``): a Python number is rounded to float32 in
front of a float32 stack, a ``numpy.float64`` scalar is not.
"""

import numpy as np


def compared_as(x, dtype):
    """The float64 number that decides ``X >= x`` / ``X < x`` for a stack of ``dtype``."""
    if np.dtype(dtype) == np.float32 and np.result_type(np.float32, x) == np.float32:
        with np.errstate(over="ignore"):
            return float(np.float32(x))
    return float(x)


def mean(X, ignore_nan=False, X_thr=None):
    X = np.asarray(X)
    if X.ndim == 2:
        X = X[None, ...]
    k, kind = X.shape[0], X.dtype.type
    with np.errstate(all="ignore"):
        if not ignore_nan and X_thr is None:
            s = np.zeros(X.shape[1:], dtype=X.dtype)
            for j in range(k):
                s = s + X[j]
            return s / kind(k)
        thr = None if X_thr is None else compared_as(X_thr, X.dtype)
        s = np.zeros(X.shape[1:], dtype=X.dtype)
        count = np.zeros(X.shape[1:], dtype=np.int64)
        for j in range(k):
            x = X[j]
            drop = np.isnan(x)
            if thr is not None:
                drop = drop | (x.astype(np.float64) < thr)
            s = s + np.where(drop, kind(0), x)
            count += ~drop
        return s / count.astype(X.dtype)


def excprob(X, X_thr, ignore_nan=False):
    X = np.asarray(X)
    scalar = np.isscalar(X_thr)
    k = X.shape[0]
    out = []
    for x_thr in [X_thr] if scalar else X_thr:
        thr = compared_as(x_thr, X.dtype)
        count = np.zeros(X.shape[1:], dtype=np.int64)
        nfinite = np.zeros(X.shape[1:], dtype=np.int64)
        for j in range(k):
            x = X[j].astype(np.float64)
            fin = np.isfinite(x)
            count += fin & (x >= thr)
            nfinite += fin
        with np.errstate(all="ignore"):
            if ignore_nan:
                p = np.where(nfinite > 0, count.astype(np.float64) / nfinite, np.nan)
            else:
                p = np.where(nfinite == k, count.astype(np.float64) / np.float64(k), np.nan)
        out.append(p)
    return out[0] if scalar else np.stack(out)
