"""The spectral STEPS member update stage by stage (csrc/steps_loop.hip, csrc/fft.hip, csrc/probmatch.hip): every
entry point of the resident update with its AR history kept as spectra, called on its own through the C API and held
against a float64 NumPy statement of the same operation (oracle/steps_spectral.py where it applies).

* psh_steps_spectral_sums_dev   Parseval sums per level; spectra with all their energy on one column (or at DC) pin
                                the Hermitian weight of that column exactly
* psh_steps_spectral_ar_dev     AR(p) on the rings + recomposition, 2p + 1 calls: every ring slot and field_spec
* psh_steps_phase_ar_dev        the reference's own domain="spectral" update, masked levels, with and without phases
* psh_mask_row_offsets_dev, psh_expand_compact_c128_dev   compact level arrays -> planes, exact
* psh_fft_irfft2_min_dev, psh_field_min_key_dev           the minimum key, read through psh_steps_mask_dev
* psh_steps_mask_probmatch_dev  against psh_steps_mask_dev followed by psh_probmatch_planned_dev, bit for bit
* the argument checks of all of them

The worst errors seen are printed (pytest -rP shows them)."""

import ctypes

import numpy as np
import pytest

from oracle import steps_spectral as oss

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (3, 5), (2, 7), (37, 53), (64, 64), (151, 189), (127, 95), (640, 710), (1226, 761)]  # (m, n)
SENTINEL = complex(7.25e300, -3.5e-300)


def _lib():
    from pysteps_amd import _lib

    return _lib


def _dev(a):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(a))


def _empty(shape, dtype):
    from pysteps_amd.device import DeviceArray

    return DeviceArray(shape, dtype)


def _host(d):
    return np.array(d.to_host(), copy=True)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _rel(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (den if den > 0 else 1.0))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype in (np.float64, np.complex128) else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _complex(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _radial(m, n, levels):
    """band-pass weights and a noise filter of the kind the nowcast builds: functions of |k|, so every spectrum built with
    them stays Hermitian (tests/test_steps_spectral_cpu.py)"""
    ky = np.fft.fftfreq(m)[:, None] * m
    kx = np.fft.rfftfreq(n)[None, :] * n
    r = np.hypot(ky, kx)
    centres = np.geomspace(1.0, max(max(m, n) / 2.5, 1.0), levels)
    w = np.stack([np.exp(-0.5 * ((np.log(np.maximum(r, 0.5)) - np.log(c)) / 0.45) ** 2) for c in centres])
    w[0][r < centres[0]] = 1.0
    noise_filter = 1.0 / (1.0 + r) ** 1.3 * (1.0 + 0.2 * np.cos(r / 3.0))
    return w, noise_filter


def _sums_ref(noise_spec, noise_filter, weights, n):
    y = noise_spec * noise_filter
    y[0, 0] = 0.0
    hw = oss.hermitian_weights(n)[None, :]
    return np.array([np.sum(hw * np.abs(y * w) ** 2) for w in weights])


def _call_sums(noise_spec_d, filter_d, weights_d, L, m, n):
    sums = _empty((L,), np.float64)
    _lib().check(_lib().lib().psh_steps_spectral_sums_dev(noise_spec_d.ptr, filter_d.ptr, weights_d.ptr, L, m, n, sums.ptr))
    return sums


# ---- 1. Parseval sums ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(4096, 4096)])
def test_spectral_sums_against_numpy(shape):
    m, n = shape
    nc = n // 2 + 1
    rng = np.random.default_rng(m * 10007 + n)
    big = m * nc > 1_000_000
    levels = (6,) if big else (1, 6, 8, 16)
    noise = _complex(rng, (m, nc))
    filt = rng.uniform(0.1, 2.0, (m, nc))
    weights = rng.random((max(levels), m, nc))
    d_noise, d_filt, d_w = _dev(noise), _dev(filt), _dev(weights)
    worst = 0.0
    for L in levels:  # the first L planes of one weights array
        got = _host(_call_sums(d_noise, d_filt, d_w, L, m, n))
        want = _sums_ref(noise, filt, weights[:L], n)
        err = np.abs(got - want) / want
        worst = max(worst, float(err.max()))
        assert err.max() <= 1e-13, (shape, L, err)
    print("spectral_sums %s: worst relative error per level %.2e" % (shape, worst))


@pytest.mark.parametrize("shape", [(2, 2), (3, 5), (2, 7), (37, 53), (64, 64), (127, 95), (151, 189), (8, 9)])
def test_spectral_sums_weigh_each_column_exactly(shape):
    """All the energy on one coefficient: the sum is exactly 1x (column 0, the Nyquist column nc - 1 of an even n),
    2x (an interior column, the last column of an odd n) or 0x (DC) of its energy - no average hides a wrong weight.
    y = 3 + 4i, filter 0.5, weights powers of two: every product is exact."""
    m, n = shape
    nc = n // 2 + 1
    L = 16
    rng = np.random.default_rng(m + 31 * n)
    filt = rng.uniform(0.1, 2.0, (m, nc))
    weights = rng.random((L, m, nc))
    scales = 2.0 ** (np.arange(L) % 5 - 2)
    spots = [((m - 1, 0), 1.0), ((0, nc - 1), 1.0 if n % 2 == 0 else 2.0), ((0, 0), 0.0)]
    if m > 1:
        spots.append(((m - 1, nc - 1), 1.0 if n % 2 == 0 else 2.0))
    if nc > 2:
        spots.append(((m // 2, 1), 2.0))
    for (r, c), mult in spots:
        noise = np.zeros((m, nc), complex)
        noise[r, c] = 3.0 + 4.0j
        f, w = filt.copy(), weights.copy()
        f[r, c] = 0.5
        w[:, r, c] = scales
        d_noise, d_filt, d_w = _dev(noise), _dev(f), _dev(w)
        got = _host(_call_sums(d_noise, d_filt, d_w, L, m, n))
        want = mult * 25.0 * 0.25 * scales**2
        assert np.array_equal(got, want), (shape, (r, c), got / (25.0 * 0.25 * scales**2))


# ---- 2. AR(p) on the spectral rings ---------------------------------------------------------------------------------
AR_CASES = [(p, L, SHAPES[(i * 5 + j) % 7]) for i, p in enumerate((1, 2, 3, 8)) for j, L in enumerate((1, 6, 16))]
AR_CASES.append((2, 6, (640, 710)))


@pytest.mark.parametrize("p,L,shape", AR_CASES)
def test_spectral_ar_against_update_spectral(p, L, shape):
    """2p + 1 successive calls with the ring head advancing modulo p: after each one every ring slot against the
    oracle's history (the slots the call must not touch unchanged bit for bit), field_spec and its DC term
    (sum_k mu_k) m n against update_spectral's recomposed spectrum."""
    lib = _lib().lib()
    m, n = shape
    nc = n // 2 + 1
    rng = np.random.default_rng(p * 1000 + L * 10 + m)
    weights = rng.random((L, m, nc))
    filt = rng.uniform(0.1, 2.0, (m, nc))
    phi = rng.uniform(-0.8, 0.8, (L, p + 1))
    noise_std, mu, sigma = rng.uniform(0.3, 1.2, L), rng.standard_normal(L) + 2.0, rng.uniform(0.2, 2.0, L)
    hist = _complex(rng, (L, p, m, nc)) * 50.0  # oldest first, as the oracle keeps it
    d_w, d_f = _dev(weights), _dev(filt)
    d_ring = _dev(hist)  # head 0: slot j holds x[j]
    d_spec = _empty((m, nc), np.complex128)
    ring_before = hist.copy()
    head = 0
    worst_ring = worst_spec = worst_dc = 0.0
    for step in range(2 * p + 1):
        white = rng.standard_normal((m, n))
        noise = np.fft.rfft2(white)
        sums = _sums_ref(noise, filt, weights, n)  # the oracle's B_k: this test isolates the AR kernel
        d_noise, d_sums = _dev(noise), _dev(sums)
        _lib().check(lib.psh_steps_spectral_ar_dev(d_ring.ptr, L, p, m, n, head, _p(phi), d_noise.ptr, d_f.ptr, d_w.ptr, d_sums.ptr,
                                                   _p(noise_std), _p(mu), _p(sigma), d_spec.ptr))
        new, total = oss.update_spectral(white, filt, weights, hist, phi, noise_std, mu, sigma, spectrum=True)
        hist = np.concatenate([hist[:, 1:], new[:, None]], axis=1)
        ring = _host(d_ring)
        for slot in range(p):
            if slot != head:
                assert _same_bits(ring[:, slot], ring_before[:, slot]), (step, slot, "a slot the call must not touch changed")
        head = (head + 1) % p
        for j in range(p):  # slot (head + j) % p holds x[j]
            for k in range(L):
                e = _rel(ring[k, (head + j) % p], hist[k, j])
                worst_ring = max(worst_ring, e)
                assert e <= 1e-12, (step, j, k, e)
        spec = _host(d_spec)
        e = _rel(spec, total)
        worst_spec = max(worst_spec, e)
        assert e <= 1e-12, (step, e)
        e = abs(spec[0, 0] - total[0, 0]) / abs(total[0, 0])
        worst_dc = max(worst_dc, e)
        assert e <= 1e-12, (step, spec[0, 0], total[0, 0])
        ring_before = ring
    print("spectral_ar p=%d L=%d %s: worst rel-L2 ring %.2e, field_spec %.2e, DC %.2e" % (p, L, shape, worst_ring, worst_spec,
                                                                                          worst_dc))


@pytest.mark.parametrize("shape", [(3, 5), (2, 7), (37, 53), (127, 95), (151, 189), (1226, 761), (4096, 4096)])
def test_spectral_chain_against_one_update_spectral_step(shape):
    """psh_steps_spectral_sums_dev -> psh_steps_spectral_ar_dev -> psh_fft_irfft2_min_dev, as the resident update chains
    them, against one update_spectral step: the new spectra and the recomposed field."""
    lib = _lib().lib()
    m, n = shape
    nc = n // 2 + 1
    L, p = 6, 2
    rng = np.random.default_rng(m + n)
    weights, filt = _radial(m, n, L)
    phi = rng.uniform(-0.8, 0.8, (L, p + 1))
    noise_std, mu, sigma = rng.uniform(0.3, 1.2, L), rng.standard_normal(L), rng.uniform(0.2, 2.0, L)
    base = np.fft.rfft2(rng.standard_normal((m, n)))
    hist = rng.uniform(0.2, 1.0, (L, p))[:, :, None, None] * base  # (4096^2: one random plane, scaled per level and slot)
    white = rng.standard_normal((m, n))
    d_w, d_f, d_noise = _dev(weights), _dev(filt), _dev(np.fft.rfft2(white))
    d_ring = _dev(hist)
    sums = _call_sums(d_noise, d_f, d_w, L, m, n)
    d_spec, field, key = _empty((m, nc), np.complex128), _empty((m, n), np.float64), _empty((1,), np.uint64)
    _lib().check(lib.psh_steps_spectral_ar_dev(d_ring.ptr, L, p, m, n, 0, _p(phi), d_noise.ptr, d_f.ptr, d_w.ptr, sums.ptr,
                                               _p(noise_std), _p(mu), _p(sigma), d_spec.ptr))
    _lib().check(lib.psh_fft_irfft2_min_dev(d_spec.ptr, m, n, field.ptr, key.ptr))
    new, want = oss.update_spectral(white, filt, weights, hist, phi, noise_std, mu, sigma)
    del hist, base
    e_ring = max(_rel(_host(d_ring.view(k).view(0)), new[k]) for k in range(L))  # slot 0 = head: the new spectra
    got = _host(field)
    e_field = _rel(got, want)
    print("spectral chain %s: rel-L2 new spectra %.2e, field %.2e" % (shape, e_ring, e_field))
    assert e_ring <= 1e-12 and e_field <= 1e-12, (e_ring, e_field)
    # the key is the field's minimum: the keep mask sets every dropped pixel to it
    keep = _dev(np.zeros((m, n), np.uint8))
    _lib().check(lib.psh_steps_mask_dev(field.ptr, m * n, None, keep.ptr, key.ptr))
    assert _same_bits(_host(field), np.full((m, n), got.min()))


# ---- 3. the reference's own domain="spectral" update ---------------------------------------------------------------
def _phase_inputs(m, n, L):
    weights, filt = _radial(m, n, L)
    nc = n // 2 + 1
    weights[weights < 1e-9] = 0.0
    weights[L // 2] = 0.0  # a level without a single coefficient
    weights[L // 2][0, 0] = 1e-12  # (not above the threshold)
    edge = np.flatnonzero(weights[1].ravel() > 1e-12)
    weights[1].ravel()[edge[:: 3]] = 1e-12  # on the threshold: not a coefficient of the level
    return weights, filt, nc


@pytest.mark.parametrize("shape,p,with_theta", [((3, 5), 1, True), ((2, 7), 2, True), ((37, 53), 2, True), ((64, 64), 3, True),
                                                 ((127, 95), 2, True), ((151, 189), 1, True), ((640, 710), 2, True),
                                                 ((37, 53), 2, False), ((127, 95), 3, False), ((64, 64), 1, False)])
def test_phase_ar_against_the_reference_spectral_update(shape, p, with_theta):
    """psh_steps_phase_ar_dev against update_reference_spectral_domain (compact levels, phases from RandomState.uniform)
    over p + 2 updates: the kept coefficients of every ring slot, the recomposed spectrum - and the sentinel the ring was
    filled with still in every entry outside a level's mask.  theta NULL: the deterministic S-PROG model (no innovation
    term; the oracle runs with the innovation coefficient at zero)."""
    lib = _lib().lib()
    m, n = shape
    L = 6
    rng = np.random.default_rng(m * 7 + n + p)
    weights, filt, nc = _phase_inputs(m, n, L)
    masks = weights > 1e-12
    counts = masks.reshape(L, -1).sum(1)
    assert counts[L // 2] == 0
    phi = rng.uniform(-0.8, 0.8, (L, p + 1))
    noise_std, mu, sigma = rng.uniform(0.3, 1.2, L), rng.standard_normal(L), rng.uniform(0.2, 2.0, L)
    compact = [_complex(rng, (p, int(c))) for c in counts]
    ring = np.full((L, p, m, nc), SENTINEL)
    for k in range(L):
        for j in range(p):
            ring[k, j][masks[k]] = compact[k][j]  # head 0: slot j holds x[j]
    d_ring, d_w, d_f = _dev(ring), _dev(weights), _dev(filt)
    d_spec = _empty((m, nc), np.complex128)
    f0 = filt.copy()
    f0[0, 0] = 0.0
    inv_std_noise = 1.0 / oss.spectral_std(f0, shape)
    with np.errstate(divide="ignore"):
        inv_std_levels = np.array([1.0 / oss.spectral_std(f0 * inv_std_noise * weights[k], shape) for k in range(L)])
    phi_oracle = phi.copy()
    if not with_theta:
        phi_oracle[:, p] = 0.0
    seed = m * 1000 + n
    oracle_rs, device_rs = np.random.RandomState(seed), np.random.RandomState(seed)
    head = 0
    worst_ring = worst_spec = 0.0
    for step in range(p + 2):
        theta = device_rs.uniform(low=0.0, high=2.0 * np.pi, size=(m, nc))  # the draw the oracle makes (it mirrors column 0)
        d_theta = _dev(theta)
        if with_theta:
            _lib().check(lib.psh_steps_phase_ar_dev(d_ring.ptr, L, p, m, n, head, _p(phi), d_theta.ptr, d_f.ptr, d_w.ptr,
                                                    inv_std_noise, _p(inv_std_levels), _p(noise_std), _p(mu), _p(sigma),
                                                    d_spec.ptr))
        else:
            _lib().check(lib.psh_steps_phase_ar_dev(d_ring.ptr, L, p, m, n, head, _p(phi), None, None, d_w.ptr, 0.0, None, None,
                                                    _p(mu), _p(sigma), d_spec.ptr))
        with np.errstate(invalid="ignore", divide="ignore"):  # the empty level: 0 / 0 on no coefficient
            want = oss.update_reference_spectral_domain(oracle_rs, shape, filt, weights, compact, phi_oracle, noise_std, mu, sigma,
                                                        spectrum=True)
        head = (head + 1) % p
        got = _host(d_ring)
        for k in range(L):
            for s in range(p):
                plane = got[k, s]
                assert _same_bits(plane[~masks[k]], np.full(int((~masks[k]).sum()), SENTINEL)), (step, k, s)
            for j in range(p):
                if counts[k]:
                    e = _rel(got[k, (head + j) % p][masks[k]], compact[k][j])
                    worst_ring = max(worst_ring, e)
                    assert e <= 1e-12, (step, k, j, e)
        e = _rel(_host(d_spec), want)
        worst_spec = max(worst_spec, e)
        assert e <= 1e-12, (step, e)
    print("phase_ar %s p=%d theta=%s: worst rel-L2 ring %.2e, field_spec %.2e" % (shape, p, with_theta, worst_ring, worst_spec))


# ---- 4. compact level arrays -> planes -------------------------------------------------------------------------------
def _compact_weights(rng, m, nc):
    w = rng.random((m, nc))
    w[rng.random((m, nc)) < 0.4] = 0.0
    w[rng.random((m, nc)) < 0.05] = 1e-12  # on the threshold: dropped
    w[m // 2] = 0.0  # a row without a kept coefficient
    if m > 2:
        w[-1] = 1.0  # a full row
    return w


@pytest.mark.parametrize("m,nc", [(1, 1), (2, 2), (3, 3), (37, 27), (64, 64), (64, 65), (151, 95), (127, 256), (33, 257),
                                  (19, 600), (1226, 381), (8192, 3)])
def test_compact_levels_expand_exactly(m, nc):
    lib = _lib().lib()
    rng = np.random.default_rng(m * 3 + nc)
    for empty in (False, True):
        w = np.zeros((m, nc)) if empty else _compact_weights(rng, m, nc)
        mask = w > 1e-12
        d_w = _dev(w)
        offsets = _empty((m + 1,), np.int32)
        _lib().check(lib.psh_mask_row_offsets_dev(d_w.ptr, m, nc, offsets.ptr))
        want = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32)
        got = _host(offsets)
        assert np.array_equal(got, want), (m, nc, empty)
        src = _complex(rng, (max(1, int(mask.sum())),))
        d_src, dst = _dev(src), _dev(np.full((m, nc), SENTINEL))  # every entry is written: zeros off the mask
        _lib().check(lib.psh_expand_compact_c128_dev(d_w.ptr, m, nc, offsets.ptr, d_src.ptr, dst.ptr))
        plane = np.zeros((m, nc), complex)
        plane[mask] = src[: int(mask.sum())]
        assert _same_bits(_host(dst), plane), (m, nc, empty)


def test_row_offsets_take_8192_rows_and_refuse_8193():
    lib, L = _lib().lib(), _lib()
    w = _dev(np.ones((8193, 2)))
    offsets = _empty((8194,), np.int32)
    assert lib.psh_mask_row_offsets_dev(w.ptr, 8193, 2, offsets.ptr) == L.PSH_EUNSUPPORTED
    L.check(lib.psh_mask_row_offsets_dev(w.ptr, 8192, 2, offsets.ptr))
    assert np.array_equal(_host(offsets)[:8193], 2 * np.arange(8193))


# ---- 5. the minimum key ----------------------------------------------------------------------------------------------
def _masked_like_numpy(field, grey, mn):
    out = mn + (field - mn) * grey
    out[~(out > mn)] = mn
    return out


def _mask_with_key(field_d, key_d, grey):
    from pysteps_amd.device import DeviceArray

    lib = _lib().lib()
    size = int(np.prod(field_d.shape))
    work = DeviceArray(field_d.shape, np.float64)
    _lib().check(lib.psh_memcpy_d2d(work.ptr, field_d.ptr, size * 8))
    d_grey = _dev(grey)
    _lib().check(lib.psh_steps_mask_dev(work.ptr, size, d_grey.ptr, None, key_d.ptr))
    return _host(work)


def _min_field(rng, m, n, at):
    f = rng.uniform(1.0, 2.0, (m, n))
    f[at] = -3.0
    return f


@pytest.mark.parametrize("shape", [(2, 2), (3, 5), (2, 7), (37, 53), (64, 64), (127, 95), (151, 189), (640, 710), (1226, 761)])
def test_irfft2_min_key_masks_like_numpy(shape):
    """psh_fft_irfft2_min_dev: the field bit for bit psh_fft_irfft2_dev's, the key equal to psh_field_min_key_dev's, and
    the masking it feeds bit for bit NumPy's with np.min - for the minimum in the first row, the last row (alone in its
    row pair for odd m), the last column, and a constant field."""
    lib = _lib().lib()
    m, n = shape
    rng = np.random.default_rng(m * n)
    grey = rng.uniform(0.0, 1.0, (m, n))
    grey[rng.random((m, n)) < 0.3] = 0.0
    const = np.zeros((m, n // 2 + 1), complex)
    const[0, 0] = 2.5 * m * n
    cases = {"first row": np.fft.rfft2(_min_field(rng, m, n, (0, n // 3))),
             "last row": np.fft.rfft2(_min_field(rng, m, n, (m - 1, n // 2))),
             "last column": np.fft.rfft2(_min_field(rng, m, n, (m // 2, n - 1))), "constant": const}
    for name, spec in cases.items():
        d_spec = _dev(spec)
        field, plain = _empty((m, n), np.float64), _empty((m, n), np.float64)
        key, key2 = _dev(np.zeros(1, np.uint64)), _dev(np.zeros(1, np.uint64))  # 0: the NaN key, below every other
        _lib().check(lib.psh_fft_irfft2_min_dev(d_spec.ptr, m, n, field.ptr, key.ptr))
        _lib().check(lib.psh_fft_irfft2_dev(d_spec.ptr, m, n, plain.ptr))
        got = _host(field)
        assert _same_bits(got, _host(plain)), (shape, name)
        _lib().check(lib.psh_field_min_key_dev(field.ptr, m * n, key2.ptr))
        assert _host(key)[0] == _host(key2)[0], (shape, name)
        want = _masked_like_numpy(got, grey, np.min(got))
        assert _same_bits(_mask_with_key(field, key, grey), want), (shape, name)
        assert _same_bits(_mask_with_key(field, key2, grey), want), (shape, name)


@pytest.mark.parametrize("shape", [(3, 5), (64, 64), (127, 95)])
def test_min_key_is_reset_by_every_call(shape):
    """Two calls in a row on one key buffer, the second field's minimum above the first's: the key is the second
    field's, not the smaller of the two."""
    lib = _lib().lib()
    m, n = shape
    rng = np.random.default_rng(m + n)
    grey = rng.uniform(0.0, 1.0, (m, n))
    first = _min_field(rng, m, n, (m - 1, 0))
    second = rng.uniform(3.0, 4.0, (m, n))
    key = _empty((1,), np.uint64)
    field = _empty((m, n), np.float64)
    s_first, s_second = _dev(np.fft.rfft2(first)), _dev(np.fft.rfft2(second))
    _lib().check(lib.psh_fft_irfft2_min_dev(s_first.ptr, m, n, field.ptr, key.ptr))
    _lib().check(lib.psh_fft_irfft2_min_dev(s_second.ptr, m, n, field.ptr, key.ptr))
    got = _host(field)
    assert got.min() > 2.9
    assert _same_bits(_mask_with_key(field, key, grey), _masked_like_numpy(got, grey, got.min()))
    d_first, d_second = _dev(first), _dev(second)
    _lib().check(lib.psh_field_min_key_dev(d_first.ptr, m * n, key.ptr))
    _lib().check(lib.psh_field_min_key_dev(d_second.ptr, m * n, key.ptr))
    assert _same_bits(_mask_with_key(d_second, key, grey), _masked_like_numpy(second, grey, second.min()))


def test_field_min_key_signed_zeros_and_nan():
    """The key orders -0.0 below +0.0 (np.min may return either zero: the values agree, the bits follow the key), and a
    NaN anywhere is the minimum (np.min propagates it)."""
    lib = _lib().lib()
    rng = np.random.default_rng(5)
    m, n = 61, 67
    grey = rng.uniform(0.0, 1.0, (m, n))
    for first_zero in (0.0, -0.0):
        f = rng.uniform(0.5, 1.0, (m, n))
        f[3, 4], f[40, 50], f[60, 66] = first_zero, -first_zero, 0.0
        key = _empty((1,), np.uint64)
        d = _dev(f)
        _lib().check(lib.psh_field_min_key_dev(d.ptr, m * n, key.ptr))
        got = _mask_with_key(d, key, grey)
        assert _same_bits(got, _masked_like_numpy(f, grey, -0.0))
        assert np.array_equal(got, _masked_like_numpy(f, grey, np.min(f)))
    f = rng.uniform(0.5, 1.0, (m, n))
    f[10, 10] = np.nan
    key = _empty((1,), np.uint64)
    d = _dev(f)
    _lib().check(lib.psh_field_min_key_dev(d.ptr, m * n, key.ptr))
    assert np.isnan(_mask_with_key(d, key, grey)).all()


# ---- 6. the mask inside the CDF matching ------------------------------------------------------------------------------
def _rain_like(rng, shape, wet):
    from scipy.ndimage import gaussian_filter

    g = gaussian_filter(rng.standard_normal(shape), 3.0)
    thr = np.quantile(g, 1.0 - wet)
    return np.where(g > thr, 10.0 * (g - thr) / g.std(), 0.0)


@pytest.mark.parametrize("shape,mask_kind", [((37, 53), "grey"), ((37, 53), "keep"), ((127, 95), "grey"), ((151, 189), "keep"),
                                             ((300, 260), "grey"), ((300, 260), "keep"), ((300, 260), "ties")])
def test_mask_probmatch_equals_mask_then_planned(shape, mask_kind):
    """psh_steps_mask_probmatch_dev against psh_steps_mask_dev followed by psh_probmatch_planned_dev: the matched field,
    the masked field left behind and the status, bit for bit - also when the matching declines (more than 16384 tied
    wet values)."""
    L_ = _lib()
    lib = L_.lib()
    m, n = shape
    count = m * n
    rng = np.random.default_rng(m + n + len(mask_kind))
    target = _rain_like(rng, shape, 0.3)
    if mask_kind == "ties":
        field = np.where(rng.random(shape) < 0.5, 1.0, -15.0)
    else:
        field = 3.0 * rng.standard_normal(shape) - 2.0
    grey = keep = None
    if mask_kind == "grey":
        grey = rng.uniform(0.0, 1.0, shape)
        grey[rng.random(shape) < 0.3] = 0.0
    else:
        keep = (rng.random(shape) < 0.9).astype(np.uint8)
    d_grey = None if grey is None else _dev(grey)
    d_keep = None if keep is None else _dev(keep)
    plan = ctypes.c_void_p()
    d_target = _dev(target)
    L_.check(lib.psh_probmatch_plan_create(d_target.ptr, count, ctypes.byref(plan)))
    try:
        d_a, d_b = _dev(field), _dev(field)
        key = _empty((1,), np.uint64)
        L_.check(lib.psh_field_min_key_dev(d_a.ptr, count, key.ptr))
        out_a, out_b = _empty(shape, np.float64), _empty(shape, np.float64)
        status = _dev(np.full(2, 12345, np.int32))
        gp, kp = (None if d_grey is None else d_grey.ptr), (None if d_keep is None else d_keep.ptr)
        L_.check(lib.psh_steps_mask_dev(d_a.ptr, count, gp, kp, key.ptr))
        L_.check(lib.psh_probmatch_planned_dev(plan, d_a.ptr, count, out_a.ptr, status.ptr))
        L_.check(lib.psh_steps_mask_probmatch_dev(plan, d_b.ptr, count, gp, kp, key.ptr, out_b.ptr, status.ptr + 4))
        st = _host(status)
        assert st[0] == st[1], st
        assert _same_bits(_host(d_a), _host(d_b))
        if mask_kind == "ties":
            assert lib.psh_probmatch_status(int(st[0])) == L_.PSH_EUNSUPPORTED
        else:
            assert st[0] == 0
            assert _same_bits(_host(out_a), _host(out_b))
    finally:
        L_.check(lib.psh_probmatch_plan_destroy(plan))


# ---- 7. argument checks ---------------------------------------------------------------------------------------------
def test_argument_checks():
    """nlevels outside 1..16 and p outside 1..8: PSH_EUNSUPPORTED; NULL pointers, ring heads outside 0..p-1, n = 1 for
    the AR kernels: PSH_EINVAL (n = 1 for the sums, like an unsupported level count: PSH_EUNSUPPORTED).  Nothing is
    launched by a refused call: every buffer is big enough for the valid call next to it."""
    L_ = _lib()
    lib = L_.lib()
    INVAL, UNSUP = L_.PSH_EINVAL, L_.PSH_EUNSUPPORTED
    m, n, p = 8, 8, 2
    nc = n // 2 + 1
    ring = _empty((16, 8, m, nc), np.complex128)
    spec, noise = _empty((m, nc), np.complex128), _empty((m, nc), np.complex128)
    filt, weights = _dev(np.ones((m, nc))), _dev(np.ones((16, m, nc)))
    sums = _empty((16,), np.float64)
    phi = np.zeros((16, 9))
    hostv = np.ones(16)
    h = _p(hostv)

    def sums_call(L=6, mm=m, nn=n, a=noise.ptr, f=filt.ptr, w=weights.ptr, s=sums.ptr):
        return lib.psh_steps_spectral_sums_dev(a, f, w, L, mm, nn, s)

    def ar_call(L=6, pp=p, mm=m, nn=n, head=0, c=ring.ptr, ph=_p(phi), a=noise.ptr, f=filt.ptr, w=weights.ptr, s=sums.ptr,
                ns=h, mu=h, sg=h, out=spec.ptr):
        return lib.psh_steps_spectral_ar_dev(c, L, pp, mm, nn, head, ph, a, f, w, s, ns, mu, sg, out)

    def phase_call(L=6, pp=p, mm=m, nn=n, head=0, c=ring.ptr, ph=_p(phi), th=filt.ptr, f=filt.ptr, w=weights.ptr, isl=h, ns=h,
                   mu=h, sg=h, out=spec.ptr):
        return lib.psh_steps_phase_ar_dev(c, L, pp, mm, nn, head, ph, th, f, w, 1.0, isl, ns, mu, sg, out)

    for L in (0, 17):
        assert sums_call(L=L) == UNSUP
        assert ar_call(L=L) == UNSUP
        assert phase_call(L=L) == UNSUP
    for pp in (0, 9):
        assert ar_call(pp=pp) == UNSUP
        assert phase_call(pp=pp) == UNSUP
    assert sums_call(nn=1) == UNSUP and sums_call(mm=0) == UNSUP
    assert ar_call(nn=1) == INVAL and ar_call(mm=0) == INVAL
    assert phase_call(nn=1) == INVAL and phase_call(mm=0) == INVAL
    for head in (-1, p):
        assert ar_call(head=head) == INVAL
        assert phase_call(head=head) == INVAL
    for arg in ("a", "f", "w", "s"):
        assert sums_call(**{arg: None}) == INVAL, arg
    for arg in ("c", "ph", "a", "f", "w", "s", "ns", "mu", "sg", "out"):
        assert ar_call(**{arg: None}) == INVAL, arg
    for arg in ("c", "ph", "w", "mu", "sg", "out", "f", "isl", "ns"):  # the last three: required with phases only
        assert phase_call(**{arg: None}) == INVAL, arg
    field = _empty((m, n), np.float64)
    key = _empty((1,), np.uint64)
    assert lib.psh_fft_irfft2_min_dev(None, m, n, field.ptr, key.ptr) == INVAL
    assert lib.psh_fft_irfft2_min_dev(spec.ptr, m, n, None, key.ptr) == INVAL
    assert lib.psh_fft_irfft2_min_dev(spec.ptr, m, n, field.ptr, None) == INVAL
    assert lib.psh_field_min_key_dev(None, m * n, key.ptr) == INVAL
    assert lib.psh_field_min_key_dev(field.ptr, m * n, None) == INVAL
    assert lib.psh_field_min_key_dev(field.ptr, 0, key.ptr) == INVAL
    offsets = _empty((m + 1,), np.int32)
    assert lib.psh_mask_row_offsets_dev(None, m, nc, offsets.ptr) == INVAL
    assert lib.psh_mask_row_offsets_dev(weights.ptr, m, nc, None) == INVAL
    assert lib.psh_mask_row_offsets_dev(weights.ptr, 0, nc, offsets.ptr) == UNSUP
    assert lib.psh_mask_row_offsets_dev(weights.ptr, m, 0, offsets.ptr) == UNSUP
    for i in range(4):
        args = [weights.ptr, offsets.ptr, noise.ptr, spec.ptr]
        args[i] = None
        assert lib.psh_expand_compact_c128_dev(args[0], m, nc, args[1], args[2], args[3]) == INVAL, i
    assert lib.psh_expand_compact_c128_dev(weights.ptr, 0, nc, offsets.ptr, noise.ptr, spec.ptr) == INVAL
    # the fused mask + matching: a plan, the field, its minimum and exactly one mask, an output of its own
    plan = ctypes.c_void_p()
    target = _dev(np.arange(m * n, dtype=np.float64))
    L_.check(lib.psh_probmatch_plan_create(target.ptr, m * n, ctypes.byref(plan)))
    try:
        grey, keep = _dev(np.ones((m, n))), _dev(np.ones((m, n), np.uint8))
        out, st = _empty((m, n), np.float64), _empty((1,), np.int32)
        assert lib.psh_steps_mask_probmatch_dev(None, field.ptr, m * n, grey.ptr, None, key.ptr, out.ptr, st.ptr) == INVAL
        assert lib.psh_steps_mask_probmatch_dev(plan, None, m * n, grey.ptr, None, key.ptr, out.ptr, st.ptr) == INVAL
        assert lib.psh_steps_mask_probmatch_dev(plan, field.ptr, m * n, grey.ptr, None, None, out.ptr, st.ptr) == INVAL
        assert lib.psh_steps_mask_probmatch_dev(plan, field.ptr, m * n, None, None, key.ptr, out.ptr, st.ptr) == INVAL
        assert lib.psh_steps_mask_probmatch_dev(plan, field.ptr, m * n, grey.ptr, keep.ptr, key.ptr, out.ptr, st.ptr) == INVAL
        assert lib.psh_steps_mask_probmatch_dev(plan, field.ptr, m * n, grey.ptr, None, key.ptr, field.ptr, st.ptr) == INVAL
        assert lib.psh_steps_mask_probmatch_dev(plan, field.ptr, m * n - 1, grey.ptr, None, key.ptr, out.ptr, st.ptr) == INVAL
    finally:
        L_.check(lib.psh_probmatch_plan_destroy(plan))
