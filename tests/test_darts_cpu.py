"""The DARTS motion estimate's host side (no GPU): argument checks, delegation, registration, and a NumPy
restatement of the reference's algebra held to the goldens (tests/golden/darts_reference.npz, written by the
unmodified reference with tools/make_golden_darts.py).  test_darts_gpu.py compares the device against
:func:`restate` where the goldens would be too large."""

import contextlib
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

RESTATE_BAR = 1e-12


def restate(frames, N_x=50, N_y=50, N_t=4, M_x=2, M_y=2, output_type="spatial", lsq_method=2, **_):
    """pysteps/motion/darts.py ``DARTS`` with its loops written as array expressions (same element arithmetic)."""
    F = np.fft.fftn(np.moveaxis(np.asarray(frames), (0, 1, 2), (2, 0, 1)))
    T_y, T_x, T_t = F.shape
    rows = (2 * N_x + 1) * (2 * N_y + 1) * (2 * N_t + 1)
    cols = (2 * M_x + 1) * (2 * M_y + 1)
    k_t, k_y, k_x = np.unravel_index(np.arange(rows), (2 * N_t + 1, 2 * N_y + 1, 2 * N_x + 1))
    k_t, k_y, k_x = k_t - N_t, k_y - N_y, k_x - N_x
    y = (k_t * F[k_y, k_x, k_t]).astype(complex)
    c1 = -1.0 * T_t / (T_x * T_y)
    kp_y, kp_x = np.unravel_index(np.arange(cols), (2 * M_y + 1, 2 * M_x + 1))
    i_ = k_y[:, None] - (kp_y - M_y)[None, :]
    j_ = k_x[:, None] - (kp_x - M_x)[None, :]
    R_ = F[i_, j_, k_t[:, None]]
    M = np.hstack([(c1 / T_y * i_) * R_, (c1 / T_x * j_) * R_]).astype(complex)
    if lsq_method == 1:
        x = np.linalg.lstsq(M, y, rcond=0.01)[0]
    else:
        M_ct = M.conjugate().T
        U, s, V = np.linalg.svd(np.dot(M_ct, M), full_matrices=False)
        s = 1.0 / s[s > 0.01 * s[0]]
        MM_inv = np.dot(np.dot(V[: len(s), :].conjugate().T, np.diag(s)), U[:, : len(s)].conjugate().T)
        x = np.dot(MM_inv, np.dot(M_ct, y))
    h, w = 2 * M_y + 1, 2 * M_x + 1
    V_ = x[: h * w].reshape(h, w)
    U_ = x[h * w : 2 * h * w].reshape(h, w)
    if output_type == "spectral":
        return np.stack([U_, V_])
    kx, ky = np.meshgrid(np.arange(-M_x, M_x + 1), np.arange(-M_y, M_y + 1))
    out = []
    for X in (U_, V_):
        X_f = np.zeros((T_y, T_x), dtype=complex)
        X_f[ky, kx] = X
        out.append(np.real(np.fft.ifft2(X_f)))
    return np.stack(out)


def rel_l2c(a, b):
    """relative L2 error for real or complex arrays"""
    a, b = np.asarray(a), np.asarray(b)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (den if den > 0 else 1.0))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "darts_reference.npz"))


def golden_case(z, name):
    """(frames in the case's dtype, keyword arguments, stored output, output stride, singular values of M^H M)"""
    frames = z["frames__" + str(z[name + "__frames"])].astype(np.float64) / 4.0
    frames = frames.astype(str(z[name + "__dtype"]))
    kw = json.loads(str(z[name + "__kwargs"]))
    return frames, kw, z[name + "__out"], int(z[name + "__stride"]), z[name + "__s"]


def golden_names(z):
    return [str(c) for c in z["cases"]]


def test_restatement_reproduces_the_goldens(golden):
    for name in golden_names(golden):
        frames, kw, want, stride, _ = golden_case(golden, name)
        got = restate(frames, **kw)
        if got.ndim == 3 and kw.get("output_type", "spatial") == "spatial":
            got = got[:, ::stride, ::stride]
        assert got.shape == want.shape, name
        assert rel_l2c(got, want) <= RESTATE_BAR, (name, rel_l2c(got, want))


def test_goldens_cover_the_cutoff(golden):
    """at least one case drops singular values at 0.01 s[0]; none lies near the cutoff"""
    dropped = 0
    for name in golden_names(golden):
        s = golden_case(golden, name)[4]
        dropped += int(np.sum(~(s > 0.01 * s[0])))
        assert np.all(np.abs(s - 0.01 * s[0]) > 1e-6 * 0.01 * s[0]), name
    assert dropped > 0


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the HIP library fails the test: the checks and the delegation decision come first."""
    from pysteps_amd import _lib

    def refuse():
        raise AssertionError("the device was used before the argument checks")

    monkeypatch.setattr(_lib, "lib", refuse)


def _value_errors():
    ok = np.zeros((6, 64, 64))
    bad = ok.copy()
    bad[2, 3, 4] = np.nan
    return [
        (np.zeros((64, 64)), {}),
        (ok, {"N_t": 5}),
        (ok[:4], {}),
        (ok, {"output_type": "dense"}),
        (bad, {}),
        (np.where(bad == bad, 0.0, np.inf), {}),
    ]


def _index_errors():
    return [
        (np.zeros((6, 40, 64)), {}),
        (np.zeros((6, 64, 40)), {}),
        (np.zeros((6, 52, 64)), {}),
        (np.zeros((6, 64, 52)), {}),
        (np.zeros((5, 30, 40)), {"N_x": 20, "N_y": 30, "N_t": 2, "M_x": 3, "M_y": 1}),
    ]


@pytest.mark.parametrize("frames,kw", _value_errors())
def test_value_errors_before_device(no_device, ref_pysteps, frames, kw):
    from pysteps.motion.darts import DARTS as ref

    from pysteps_amd.motion.darts import DARTS

    with pytest.raises(ValueError) as want:
        ref(frames, verbose=False, **kw)
    with pytest.raises(ValueError) as got:
        DARTS(frames, verbose=False, **kw)
    assert str(got.value) == str(want.value)


@pytest.mark.parametrize("frames,kw", _index_errors())
def test_index_errors_before_device(no_device, ref_pysteps, frames, kw):
    from pysteps.motion.darts import DARTS as ref

    from pysteps_amd.motion.darts import DARTS

    with pytest.raises(IndexError) as want:
        ref(frames, verbose=False, **kw)
    with pytest.raises(IndexError) as got:
        DARTS(frames, verbose=False, **kw)
    assert str(got.value) == str(want.value)


def test_smallest_valid_size_raises_nothing_on_the_host():
    from pysteps_amd.motion import darts

    o = darts._options({})
    darts._raise_index_error((53, 53, 6), o)
    with pytest.raises(IndexError):
        darts._raise_index_error((52, 53, 6), o)


def test_unsupported_shape_delegates(no_device, ref_pysteps):
    from pysteps.motion.darts import DARTS as ref

    from pysteps_amd.motion.darts import DARTS

    rng = np.random.default_rng(5)
    frames = rng.random((6, 4100, 54)) * 10.0
    kw = dict(N_x=2, N_y=2, N_t=1)
    with contextlib.redirect_stdout(io.StringIO()):
        want = ref(frames.copy(), **kw)
        with pytest.warns(UserWarning, match="not taken by the device FFT"):
            got = DARTS(frames.copy(), **kw)
    assert np.array_equal(got, want)


def test_unsupported_without_pysteps_raises(no_device, monkeypatch):
    from pysteps_amd.motion import darts

    monkeypatch.setattr(darts, "lookup", lambda module, name, ours: None)
    with pytest.raises(NotImplementedError, match="device FFT"):
        darts.DARTS(np.zeros((6, 4100, 54)), verbose=False)


def test_register_into_adds_darts_hip():
    from pysteps_amd import register
    from pysteps_amd.motion.darts import DARTS

    stock = object()
    for override in (False, True):
        motion = {"darts": stock}
        added = register.register_into(motion, None, override=override)
        assert "motion:darts_hip" in added
        assert motion["darts_hip"] is DARTS
        assert motion["darts"] is stock


def test_package_table():
    from pysteps_amd import motion
    from pysteps_amd.motion.darts import DARTS

    assert motion.get_method("darts_hip") is DARTS
    assert motion.get_method("DARTS_HIP") is DARTS


def test_pysteps_tables(ref_pysteps):
    import pysteps.motion as ref_motion
    import pysteps.motion.interface as mot_if

    from pysteps_amd import motion, register
    from pysteps_amd.motion.darts import DARTS

    stock = ref_motion.get_method("darts")
    assert stock is not DARTS and motion.get_method("darts") is stock
    saved = dict(mot_if._methods)
    try:
        for override in (False, True):
            register.register_into(mot_if._methods, None, override=override)
            assert ref_motion.get_method("darts_hip") is DARTS
            assert ref_motion.get_method("darts") is stock and motion.get_method("darts") is stock
    finally:
        mot_if._methods.clear()
        mot_if._methods.update(saved)
