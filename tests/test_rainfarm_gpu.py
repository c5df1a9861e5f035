"""RainFARM downscaling on the device (pysteps_amd/downscaling/rainfarm.py, csrc/rainfarm.hip) against the unmodified
reference's goldens (tools/make_golden_rainfarm.py) and the long-double restatement (helpers/rainfarm.py).

No bar comes from the code under test.  The golden file carries the reference's own deviations from the long-double
restatement - ``deviation_noise`` (in u = 2^-53 rms per pixel), ``deviation_finish``, ``deviation_field`` (largest
absolute difference over the case's largest output value) and ``deviation_alpha``; tests/golden/fft_pointwise_bars.json
carries the bar ``B`` of the transform used (``irfft2``) for the shape's class.  Every test prints what it saw next to
its bar.
"""

import builtins
import functools
import json
import warnings

import numpy as np
import pytest

from helpers import fft_pointwise as fp
from helpers import rainfarm as rf

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in rf.CASES]
CASE = {c[0]: c for c in rf.CASES}
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    return rf.load_golden()


@pytest.fixture(scope="module")
def fft_bars():
    return fp.load_bars()


@functools.lru_cache(maxsize=None)
def material(name):
    """(precip, uniforms, the float64 restatement's noise field at the golden's alpha) - computed once per case."""
    g = rf.load_golden()
    _, shape, ds, _, _, seed = CASE[name]
    u = rf.draw(seed, (shape[0] * ds, shape[1] * ds))
    u.setflags(write=False)
    precip = g[name + "__precip"]
    noise = rf.noise_field(u, float(g[name + "__alpha"]), shape, ds)
    noise.setflags(write=False)
    return precip, u, noise


def transform_bar(fft_bars, name):
    _, shape, ds, _, _, _ = CASE[name]
    return fp.bar(fft_bars, fp.shape_class((shape[0] * ds, shape[1] * ds)), "irfft2")


def field_bar(golden, fft_bars, name):
    """5 x deviation_field + 2 (1 + g) B 2^-53: the second term is what a per-pixel noise error of B u can do to
    exp(noise / std) and to the aggregate it is divided by."""
    g = float(golden[name + "__g"])
    return rf.BAR_FACTOR * float(golden["deviation_field"]) + 2 * (1 + g) * transform_bar(fft_bars, name) * EPS


def strided(golden, name, x):
    s = int(golden[name + "__stride"])
    return np.asarray(x)[::s, ::s]


@pytest.mark.parametrize("name", NAMES)
def test_draw_and_generator_state(golden, name):
    """The device's uniforms are RandomState(seed).rand(M, N) bit for bit; after a call the generator handed over - and
    the global one with randstate=None - is where that one host draw leaves it."""
    from pysteps_amd.downscaling.rainfarm import downscale
    from pysteps_amd.noise.randstate import DeviceRandomStates

    _, shape, ds, kernel, _, seed = CASE[name]
    precip, u, _ = material(name)
    M, N = u.shape
    host = np.random.RandomState(seed)
    host.rand(M, N)
    after = host.get_state()

    rs = np.random.RandomState(seed)
    gen = DeviceRandomStates([rs], M * N)
    got = gen.uniform(0.0, 1.0, M, N).to_host()[0]
    gen.close()
    assert np.array_equal(got, u)

    def same(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]

    rs = np.random.RandomState(seed)
    downscale(precip, ds, alpha=1.5, kernel_type=kernel, randstate=rs)
    assert same(rs.get_state(), after)

    saved = np.random.get_state()
    try:
        np.random.seed(seed)
        downscale(precip, ds, alpha=1.5, kernel_type=kernel)
        assert same(np.random.get_state(), after)
    finally:
        np.random.set_state(saved)


@pytest.mark.parametrize("name", NAMES)
def test_noise_field(golden, fft_bars, name):
    """noise_field against the long-double restatement, per pixel in u: within 5 x deviation_noise + B; finite; its mean
    zero to the same bar (the DC bin is written as 0)."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.downscaling.rainfarm import noise_field

    _, shape, ds, _, _, _ = CASE[name]
    _, u, _ = material(name)
    alpha = float(golden[name + "__alpha"])
    got = noise_field(DeviceArray.from_host(u), alpha, shape, ds).to_host()
    want = rf.noise_field(u, alpha, shape, ds, np.longdouble)
    bar = rf.BAR_FACTOR * float(golden["deviation_noise"]) + transform_bar(fft_bars, name)
    err, at = fp.compare(got, want)
    mean_u = abs(float(np.mean(got.astype(np.longdouble)))) / fp.unit(want)
    print("%s: noise field %.1f u at %s, mean %.2f u (bar %.1f u)" % (name, err, at, mean_u, bar))
    assert np.isfinite(got).all()
    assert err <= bar
    assert mean_u <= bar


@pytest.mark.parametrize("name", NAMES)
def test_finish_stage(golden, name):
    """finish on a noise field uploaded from the host (the float64 restatement's, which is the reference's bit for bit:
    tests/test_rainfarm_cpu.py) against the golden.  Bar: 5 x deviation_finish; with a smoothing kernel that comes out
    below ((2r+1)^2 - 1) 2^-53 - the derived bound for summing that many terms in another order (the device sums
    per coarse cell, the reference through an FFT convolution) - so that bound is the bar there.  Without a kernel
    the ds x ds block means of the output equal the input within the same bar."""
    from pysteps_amd.downscaling.rainfarm import finish

    _, shape, ds, kernel, _, _ = CASE[name]
    precip, _, noise = material(name)
    got = finish(precip, np.array(noise), ds, kernel, None, np.float64).to_host()
    bar = rf.BAR_FACTOR * float(golden["deviation_finish"])
    if kernel:
        r = rf.kernel_radius(ds)
        bar = max(bar, ((2 * r + 1) ** 2 - 1) * EPS)
    want = golden[name + "__out"]
    diff = rf.scaled_diff(strided(golden, name, got), want)
    print("%s: finish %.3g (bar %.3g)" % (name, diff, bar))
    assert got.shape == noise.shape and np.isfinite(got).all()
    assert diff <= bar
    if not kernel:
        m, n = shape
        means = got.reshape(m, ds, n, ds).mean(axis=(1, 3))
        off = float(np.abs(means - precip).max() / np.abs(got).max())
        print("%s: block means vs input %.3g (bar %.3g)" % (name, off, bar))
        assert off <= bar


@pytest.mark.parametrize("name", NAMES)
def test_whole_call(golden, fft_bars, name):
    """The whole call from the seed.  alpha given: against the golden.  alpha=None: the returned alpha within
    5 x deviation_alpha of the golden's, the field against the float64 restatement evaluated at the alpha the device
    returned.  Bar: field_bar()."""
    from pysteps_amd.downscaling.rainfarm import downscale

    _, shape, ds, kernel, alpha, seed = CASE[name]
    precip, u, _ = material(name)
    bar = field_bar(golden, fft_bars, name)
    rs = np.random.RandomState(seed)
    if alpha is not None:
        got, a = downscale(precip, ds, alpha=alpha, kernel_type=kernel, return_alpha=True, randstate=rs)
        assert a == alpha
        want = golden[name + "__out"]
        got = strided(golden, name, got)
    else:
        got, a = downscale(precip, ds, kernel_type=kernel, return_alpha=True, randstate=rs)
        a_bar = rf.BAR_FACTOR * float(golden["deviation_alpha"])
        a_off = abs(float(a) - float(golden[name + "__alpha"]))
        print("%s: alpha %.15g, off the golden's by %.3g (bar %.3g)" % (name, a, a_off, a_bar))
        assert a_off <= a_bar
        want = rf.pipeline(precip, u, ds, float(a), kernel)
    diff = rf.scaled_diff(got, want)
    print("%s: field %.3g (bar %.3g)" % (name, diff, bar))
    assert got.dtype == np.float64 and np.isfinite(got).all()
    assert diff <= bar


@pytest.mark.parametrize("name", rf.THRESHOLD_CASES)
@pytest.mark.parametrize("which", ["0.1", "median"])
def test_threshold(golden, fft_bars, name, which):
    """The thresholded result is where(x < thr, 0, x) of the device's own unthresholded result bit for bit, and equals
    the golden's thresholded field wherever the golden's value is farther from thr than the bar (at most 0.1 % of the
    pixels may be left out this way)."""
    from pysteps_amd.downscaling.rainfarm import downscale

    _, shape, ds, kernel, _, seed = CASE[name]
    precip, _, _ = material(name)
    alpha = float(golden[name + "__alpha"])
    gold = golden[name + "__out"]
    thr = 0.1 if which == "0.1" else float(np.median(gold[gold > 0]))
    plain = downscale(precip, ds, alpha=alpha, kernel_type=kernel, randstate=np.random.RandomState(seed))
    got = downscale(precip, ds, alpha=alpha, kernel_type=kernel, threshold=thr, randstate=np.random.RandomState(seed))
    assert np.array_equal(got, np.where(plain < thr, 0.0, plain))
    bar = field_bar(golden, fft_bars, name) * float(np.abs(gold).max())
    decided = np.abs(gold - thr) > bar
    left_out = int(np.count_nonzero(~decided))
    print("%s thr %.6g: %d of %d pixels within the bar of the threshold" % (name, thr, left_out, gold.size))
    assert left_out <= rf.THRESHOLD_SKIP_SHARE * gold.size
    want = np.where(gold < thr, 0.0, gold)
    g = strided(golden, name, got)
    assert np.array_equal((g == 0)[decided], (want == 0)[decided])
    assert np.abs(g - want)[decided].max() <= bar


def test_forms_resident_float32_and_repeat(golden):
    """A resident float64 call equals the NumPy call bit for bit, a resident float32 call that result rounded to
    float32; two runs of the same call are bit-identical."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.downscaling.rainfarm import downscale

    name = "chirp_20x27_ds3_gauss"
    _, shape, ds, kernel, _, seed = CASE[name]
    precip, _, _ = material(name)
    assert np.array_equal(precip.astype(np.float32).astype(np.float64), precip)
    kw = dict(kernel_type=kernel, threshold=0.05, return_alpha=True)
    host, a = downscale(precip, ds, randstate=np.random.RandomState(seed), **kw)
    again, a2 = downscale(precip, ds, randstate=np.random.RandomState(seed), **kw)
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and host.shape == (shape[0] * ds, shape[1] * ds)
    assert np.array_equal(host, again) and a == a2
    res, a3 = downscale(DeviceArray.from_host(precip), ds, randstate=np.random.RandomState(seed), **kw)
    assert isinstance(res, DeviceArray) and res.dtype == np.float64 and a3 == a
    assert np.array_equal(res.to_host(), host)
    res32, a4 = downscale(DeviceArray.from_host(precip.astype(np.float32)), ds, randstate=np.random.RandomState(seed), **kw)
    assert isinstance(res32, DeviceArray) and res32.dtype == np.float32 and a4 == a
    assert np.array_equal(res32.to_host(), host.astype(np.float32))
    # a float32 NumPy field is widened: float64 out, the same values
    host32 = downscale(precip.astype(np.float32), ds, randstate=np.random.RandomState(seed), **kw)[0]
    assert host32.dtype == np.float64 and np.array_equal(host32, host)


def test_downscale_table(golden):
    """downscale_table of a 3-plane stack equals three successive calls bit for bit and leaves the generator where they
    do; one field with n_realizations=3 likewise; a plane's bits do not depend on its position in the stack."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.downscaling.rainfarm import downscale, downscale_table

    ds, kernel = 3, "gaussian"
    stack = np.stack([rf.field((20, 27), s) for s in (102, 202, 302)])
    rs = np.random.RandomState(11)
    singles = [downscale(p, ds, kernel_type=kernel, return_alpha=True, randstate=rs) for p in stack]
    after = rs.get_state()
    rs = np.random.RandomState(11)
    table, alphas = downscale_table(stack, ds, kernel_type=kernel, return_alpha=True, randstate=rs)
    assert table.shape == (3, 60, 81) and table.dtype == np.float64
    for j in range(3):
        assert np.array_equal(table[j], singles[j][0]) and alphas[j] == singles[j][1]
    st = rs.get_state()
    assert np.array_equal(st[1], after[1]) and st[2:] == after[2:]

    rs = np.random.RandomState(12)
    singles = [downscale(stack[0], ds, alpha=2.0, randstate=rs) for _ in range(3)]
    rs = np.random.RandomState(12)
    res = downscale_table(DeviceArray.from_host(stack[0]), ds, n_realizations=3, alpha=2.0, randstate=rs)
    assert isinstance(res, DeviceArray) and res.shape == (3, 60, 81)
    res = res.to_host()
    for j in range(3):
        assert np.array_equal(res[j], singles[j])


def test_finish_table_wider_than_three_cells():
    """The reference's radius rule always gives a 3 x 3 cell table, which the finish kernel is specialised for.  A
    wider kernel (radius 4 at ds = 2: 5 x 5 cells, clipped on every side of a 3 x 4 field) goes through the kernel's
    general path: with E = 1 the output is S(P) / S(A), held to the plain tap loop on the host within
    ((2r+1)^2 - 1) 2^-53 per average."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.downscaling.rainfarm import weight_table

    ds, r, (m, n) = 2, 4, (3, 4)
    x = np.arange(-r, r + 1)
    k1 = np.exp(-0.5 / 4.0 * x**2)
    kernel = np.outer(k1, k1)
    kernel[0, 0] = kernel[-1, -1] = kernel[0, -1] = kernel[-1, 0] = 0.0  # not an outer product
    kernel /= kernel.sum()
    table, amin = weight_table(kernel, ds)
    assert table.shape == (ds, ds, 5, 5) and amin == -2
    rng = np.random.RandomState(4)
    P, A = rng.rand(m, n) + 0.5, rng.rand(m, n) + 0.5
    ones = np.ones((ds, ds))
    want = rf.balanced_average(np.kron(P, ones), kernel, True) / rf.balanced_average(np.kron(A, ones), kernel, True)
    out = DeviceArray((1, m * ds, n * ds), np.float64)
    e = DeviceArray.from_host(np.ones((1, m * ds, n * ds)))
    dP, dA, dT = DeviceArray.from_host(P), DeviceArray.from_host(A), DeviceArray.from_host(table)
    _lib.check(_lib.lib().psh_rainfarm_finish_dev(e.ptr, dP.ptr, 1, dA.ptr, 1, m, n, ds, dT.ptr, 5, amin, 0, 0.0, 0, out.ptr),
               "psh_rainfarm_finish_dev")
    got = out.to_host()[0]
    bar = 3 * ((2 * r + 1) ** 2 - 1) * EPS  # two averages and their quotient
    diff = rf.scaled_diff(got, want)
    print("5 x 5 cell table: %.3g (bar %.3g)" % (diff, bar))
    assert diff <= bar


def test_callers_device_generator():
    """A DeviceRandomStates handle the caller keeps gives, call after call, what successive calls on the host generator
    give, bit for bit; its sync_back() leaves the host generator where they leave it."""
    from pysteps_amd.downscaling.rainfarm import downscale
    from pysteps_amd.noise.randstate import DeviceRandomStates

    precip = rf.field((16, 32), 101)
    rs = np.random.RandomState(21)
    want = [downscale(precip, 4, alpha=1.6, kernel_type="tophat", randstate=rs) for _ in range(3)]
    after = rs.get_state()
    rs = np.random.RandomState(21)
    gen = DeviceRandomStates([rs], 64 * 128)
    try:
        got = [downscale(precip, 4, alpha=1.6, kernel_type="tophat", randstate=gen) for _ in range(3)]
        gen.sync_back()
        with pytest.raises(ValueError):
            downscale(precip, 8, alpha=1.6, randstate=gen)  # max_draw too small
    finally:
        gen.close()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    st = rs.get_state()
    assert np.array_equal(st[1], after[1]) and st[2:] == after[2:]


def test_spectral_fusion_goes_to_the_reference(ref_pysteps):
    """spectral_fusion=True warns, names the reason and returns the reference's result."""
    from pysteps.downscaling import rainfarm as ref

    from pysteps_amd.downscaling.rainfarm import downscale

    precip = rf.field((32, 32), 106)
    saved = np.random.get_state()
    try:
        np.random.seed(5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = ref.downscale(precip.copy(), 2, spectral_fusion=True)
        np.random.seed(5)
        with pytest.warns(RuntimeWarning, match="spectral_fusion"):
            got = downscale(precip.copy(), 2, spectral_fusion=True)
        assert np.array_equal(got, want, equal_nan=True)
        with pytest.warns(RuntimeWarning, match="spectral_fusion"):
            got = downscale(precip.copy(), 2, spectral_fusion=True, randstate=np.random.RandomState(5))
        assert np.array_equal(got, want, equal_nan=True)
    finally:
        np.random.set_state(saved)


def test_dry_field_and_resident_nonfinite(golden):
    """An all-dry field with alpha=None raises what the reference raises, and leaves the generator alone; a resident
    field is checked for non-finite values on the device."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.downscaling.rainfarm import downscale

    exc = getattr(builtins, str(golden["dry_exception"]))
    rs = np.random.RandomState(3)
    before = rs.get_state()
    with np.errstate(all="ignore"), pytest.raises(exc):
        downscale(np.zeros((8, 8)), 2, randstate=rs)
    assert np.array_equal(rs.get_state()[1], before[1]) and rs.get_state()[2] == before[2]
    bad = np.ones((8, 8))
    bad[3, 4] = np.inf
    with pytest.raises(ValueError) as e:
        downscale(DeviceArray.from_host(bad), 2, alpha=1.0)
    assert str(e.value) == json.loads(str(golden["messages"]))["nonfinite"]
