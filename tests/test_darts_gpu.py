"""The DARTS motion estimate on the device (``pysteps_amd.motion.get_method("darts_hip")``, csrc/darts.hip).

Whole calls are held to tests/golden/darts_reference.npz (the unmodified reference's outputs, written by
tools/make_golden_darts.py) and, at sizes the goldens cannot hold, to the NumPy restatement of test_darts_cpu.py
(itself held to the goldens at 1e-12).  The device computes the spectrum as rfft2 per frame plus a DFT along time
and reduces M^H M in its own order, so it differs from NumPy by rounding only: relative L2 <= REL_BAR.  The float32
case runs in float64 on the device; the reference's float32 run (complex64 FFT) is met within F32_REF_BAR.
Stages: the band cube against numpy.fft.fftn bins, the row matrix bit for bit against NumPy on the same cube, the
normal equations and the synthesis against NumPy.
"""

import contextlib
import io
import re

import numpy as np
import pytest

from test_darts_cpu import golden, golden_case, golden_names, rel_l2c, restate  # noqa: F401

pytestmark = pytest.mark.gpu

# worst seen on an MI355X: rel-L2 3.5e-14 (cutoff); the bars are 5x the worst seen
REL_BAR = 2e-13
# the reference's complex64 FFT of float32 frames: 4.8e-8 from the device's float64 result
F32_REF_BAR = 2.5e-7


def darts():
    from pysteps_amd.motion import get_method

    return get_method("darts_hip")


def dev(a):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(a))


def _cases():
    import os

    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "darts_reference.npz"))
    return [c for c in golden_names(z) if c != "float32_as_f64"]


@pytest.mark.parametrize("name", _cases())
def test_golden_case(golden, name):  # noqa: F811
    frames, kw, want, stride, s = golden_case(golden, name)
    assert np.all(np.abs(s - 0.01 * s[0]) > 1e-6 * 0.01 * s[0]), "a singular value lies at the cutoff"
    kw = dict(kw, verbose=False)
    got = darts()(frames, **kw)
    assert isinstance(got, np.ndarray)
    if kw.get("output_type", "spatial") == "spatial":
        assert got.dtype == np.float64 and got.shape == (2,) + frames.shape[1:]
        got = got[:, ::stride, ::stride]
    else:
        assert got.dtype == np.complex128
    err = rel_l2c(got, want)
    print("darts golden %s rel-L2 %.3e" % (name, err))
    if name == "float32":
        assert err <= F32_REF_BAR, err
        want64 = golden_case(golden, "float32_as_f64")[2]
        err = rel_l2c(got, want64)
        print("darts golden float32_as_f64 rel-L2 %.3e" % err)
    assert err <= REL_BAR, err


def _band_bins(frames, N_y, N_x, N_t, M_y, M_x):
    F = np.fft.fftn(np.moveaxis(frames, (0, 1, 2), (2, 0, 1)))
    m, n, T = F.shape
    ky, kx = N_y + M_y, N_x + M_x
    iy = (np.arange(-ky, ky + 1) % m)[None, :, None]
    ix = (np.arange(-kx, kx + 1) % n)[None, None, :]
    it = (np.arange(-N_t, N_t + 1) % T)[:, None, None]
    return F[iy, ix, it]


@pytest.mark.parametrize("shape,kw", [((6, 128, 128), {}), ((6, 64, 80), {}), ((5, 53, 61), dict(N_t=2)),
                                      ((9, 201, 333), dict(N_x=20, N_y=30, M_x=3, M_y=1))])
def test_band_cube(shape, kw):
    """every bin the reference reads, aliased (64 x 80: 2 K + 1 > side) and Hermitian-rebuilt ones included"""
    from pysteps_amd.motion import darts as mod

    o = mod._options(kw)
    frames = np.random.default_rng(1).random(shape) * 30.0
    cube = mod.band_cube(dev(frames), o["N_y"], o["N_x"], o["N_t"], o["M_y"], o["M_x"]).to_host()
    want = _band_bins(frames, o["N_y"], o["N_x"], o["N_t"], o["M_y"], o["M_x"])
    assert cube.shape == want.shape
    assert np.max(np.abs(cube - want)) <= 1e-13 * np.max(np.abs(want))
    wide = mod.band_cube(dev(frames.astype(np.float32)), o["N_y"], o["N_x"], o["N_t"], o["M_y"], o["M_x"]).to_host()
    want32 = _band_bins(frames.astype(np.float32).astype(np.float64), o["N_y"], o["N_x"], o["N_t"], o["M_y"], o["M_x"])
    assert np.max(np.abs(wide - want32)) <= 1e-13 * np.max(np.abs(want32))


def _rows_from_cube(cube, shape, N_x, N_y, N_t, M_x, M_y):
    """M and y of the reference, indexed into the band cube, with the reference's element arithmetic"""
    T_t, T_y, T_x = shape
    rows = (2 * N_x + 1) * (2 * N_y + 1) * (2 * N_t + 1)
    cols = (2 * M_x + 1) * (2 * M_y + 1)
    K_y, K_x = N_y + M_y, N_x + M_x
    k_t, k_y, k_x = np.unravel_index(np.arange(rows), (2 * N_t + 1, 2 * N_y + 1, 2 * N_x + 1))
    k_t, k_y, k_x = k_t - N_t, k_y - N_y, k_x - N_x
    y = k_t * cube[k_t + N_t, k_y + K_y, k_x + K_x]
    c1 = -1.0 * T_t / (T_x * T_y)
    kp_y, kp_x = np.unravel_index(np.arange(cols), (2 * M_y + 1, 2 * M_x + 1))
    i_ = k_y[:, None] - (kp_y - M_y)[None, :]
    j_ = k_x[:, None] - (kp_x - M_x)[None, :]
    R_ = cube[(k_t + N_t)[:, None], i_ + K_y, j_ + K_x]
    return np.hstack([(c1 / T_y * i_) * R_, (c1 / T_x * j_) * R_]), y


@pytest.mark.parametrize("shape,kw", [((6, 96, 96), {}), ((5, 64, 80), dict(N_x=20, N_y=30, N_t=2, M_x=3, M_y=1))])
def test_rows_and_normal_equations(shape, kw):
    from pysteps_amd.motion import darts as mod

    o = mod._options(kw)
    frames = np.random.default_rng(2).random(shape) * 30.0
    cube_d = mod.band_cube(dev(frames), o["N_y"], o["N_x"], o["N_t"], o["M_y"], o["M_x"])
    M, y = _rows_from_cube(cube_d.to_host(), shape, o["N_x"], o["N_y"], o["N_t"], o["M_x"], o["M_y"])
    M_d, y_d = mod.row_matrix(cube_d, shape, o)
    assert np.array_equal(M_d.to_host(), M) and np.array_equal(y_d.to_host(), y)
    MM, Mhy = mod.gram(cube_d, shape, o)
    M_ct = M.conjugate().T
    assert rel_l2c(MM, np.dot(M_ct, M)) <= 1e-13
    assert rel_l2c(Mhy, np.dot(M_ct, y)) <= 1e-13
    assert np.array_equal(MM, MM.conjugate().T)  # the same products in the same order
    MM2, Mhy2 = mod.gram(cube_d, shape, o)
    assert np.array_equal(MM, MM2) and np.array_equal(Mhy, Mhy2)


@pytest.mark.parametrize("m,n,M_y,M_x", [(4, 5, 2, 2), (3, 2, 2, 1), (96, 96, 2, 2), (300, 257, 1, 3), (1226, 761, 2, 2)])
def test_synthesis(m, n, M_y, M_x):
    """Re(ifft2(_fill(X))) of the reference, duplicate bins on tiny grids included"""
    from pysteps_amd.motion import darts as mod

    rng = np.random.default_rng(m * n)
    h, w = 2 * M_y + 1, 2 * M_x + 1
    U = rng.standard_normal((h, w)) + 1j * rng.standard_normal((h, w))
    V = rng.standard_normal((h, w)) + 1j * rng.standard_normal((h, w))
    ky, kx, vals = mod.fill_bins(U, V, m, n, M_y, M_x)
    got = mod.synthesize(ky, kx, vals, m, n).to_host()
    k_x, k_y = np.meshgrid(np.arange(-M_x, M_x + 1), np.arange(-M_y, M_y + 1))
    for c, X in enumerate((U, V)):
        X_f = np.zeros((m, n), dtype=complex)
        X_f[k_y, k_x] = X
        want = np.real(np.fft.ifft2(X_f))
        assert np.max(np.abs(got[c] - want)) <= 1e-13 * max(np.max(np.abs(want)), 1e-300), (c, m, n)


def test_resident_chain_into_semilagrangian(golden):  # noqa: F811
    from pysteps_amd import extrapolation
    from pysteps_amd.device import DeviceArray

    frames, kw, _, _, _ = golden_case(golden, "float32_as_f64")
    want = golden_case(golden, "float32_as_f64")[2]
    frames_d = dev(frames.astype(np.float32))
    field = darts()(frames_d, verbose=False)
    assert isinstance(field, DeviceArray) and field.shape == (2,) + frames.shape[1:] and field.dtype == np.float32
    host = field.to_host().astype(np.float64)[:, ::4, ::4]
    assert rel_l2c(host, want) <= 1e-6  # float32 rounding of the field
    f64 = darts()(dev(frames), verbose=False)
    assert isinstance(f64, DeviceArray) and f64.dtype == np.float64
    assert rel_l2c(f64.to_host()[:, ::4, ::4], want) <= REL_BAR
    last = DeviceArray.from_host(frames[-1].astype(np.float32))
    adv = extrapolation.get_method("semilagrangian")(last, field, 2)
    assert isinstance(adv, DeviceArray) and adv.shape == (2,) + frames.shape[1:]
    ref = extrapolation.get_method("semilagrangian")(frames[-1].astype(np.float32), field.to_host(), 2)
    assert np.allclose(np.asarray(adv.to_host()), np.asarray(ref), rtol=0.0, atol=1e-5, equal_nan=True)
    spec = darts()(frames_d, verbose=False, output_type="spectral")
    assert isinstance(spec, DeviceArray) and spec.dtype == np.complex128 and spec.shape == (2, 5, 5)


def test_nonfinite_resident_input_raises():
    frames = np.zeros((6, 64, 64), np.float32)
    frames[3, 10, 20] = np.inf
    with pytest.raises(ValueError, match="the input images contain non-finite values"):
        darts()(dev(frames), verbose=False)


def test_bit_identical_runs(golden):  # noqa: F811
    frames = golden_case(golden, "defaults_128")[0]
    a = darts()(frames, verbose=False)
    b = darts()(frames, verbose=False)
    assert np.array_equal(a, b)


def test_verbose_text(golden):  # noqa: F811
    frames = golden_case(golden, "defaults_128")[0]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        darts()(frames)
    text = re.sub(r"Done in [0-9.]+ seconds\.", "Done in <t> seconds.", buf.getvalue())
    text = re.sub(r"--- [0-9.eE+-]+ seconds ---", "--- <t> seconds ---", text)
    assert text == str(golden["defaults_128__text"])


@pytest.mark.parametrize("m,n", [(4096, 4096), (1226, 761)])
def test_full_size_against_restatement(m, n):
    from tools import synth

    frames = np.maximum(synth.steps_frames(m, n, n_frames=6, seed=21).astype(np.float64) + 15.0, 0.0)
    got = darts()(dev(frames), verbose=False).to_host()
    want = restate(frames)
    err = rel_l2c(got, want)
    print("darts full size %dx%d rel-L2 %.3e" % (m, n, err))
    assert err <= REL_BAR, err
