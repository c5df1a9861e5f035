"""psh_init -> operations -> psh_shutdown, three times in one process (run by tests/test_shutdown_gpu.py in a child).

Every cycle runs the same operations on the same inputs - one per device resource the library keeps for itself - and
copies the results to plain host memory; before the shutdown every DeviceArray and handle is dropped.  Cycle 1 is held
to the oracle of each operation at the bar of that operation's own test, cycles 2 and 3 to cycle 1 bit for bit.  In
cycle 2 one psh_malloc block and one psh_host_alloc block are held across the shutdown and freed after the next
psh_init.  Exit status 0 only if all of that held; `hbm_free` after each psh_init is printed, not judged.
"""

import ctypes
import gc
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pysteps_amd import _lib  # noqa: E402
from pysteps_amd.device import DeviceArray  # noqa: E402

NAN = float("nan")


def _host(dev):
    return np.array(dev.to_host(), copy=True)  # never a view of a pinned block: those end with the shutdown


def _inputs():
    from tools import synth

    rng = np.random.default_rng(2026)
    inp = {}
    for m, n in ((72, 104), (64, 96)):
        inp["sl", m, n] = (synth.rain_field_db(m, n, seed=m), synth.true_velocity(m, n))
    base = synth.rain_field_db(256, 256, seed=258, sigma=256 / 96.0)
    from oracle import semilag_cport as ocl

    adv = ocl.extrapolate(base, synth.true_velocity(256, 256), 1, outval=-15.0)
    inp["lk"] = np.stack([base, adv[0]])
    inp["corner"] = synth.rain_field_db(128, 160, seed=7 + 128, sigma=2.0)
    for shape in ((64, 64), (17, 31)):
        inp["fft", shape] = rng.standard_normal(shape) * 3 + 1.5
    g = rng.standard_normal((1, 77))
    inp["mask"] = (g, float(np.quantile(g, 0.8)), np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8), 3)
    initial = rng.normal(size=(64, 64)) * 5
    initial[initial < -2.0] = -15.0
    # (+ 0.0: no negative zeros - they tie with the positive ones, and which of two tied target values lands on which
    # rank is not fixed, so the bytes of the result would not be either)
    inp["pm"] = (initial, np.round(rng.normal(size=(64, 64)) * 6, 1) + 0.0)
    return inp


def _semilag_dev(lib, p, v, T=3):
    m, n = p.shape
    assert lib.psh_semilag_kernel(m, n, T, 1, 1, 1) == 12, "the window kernel must be the one chosen"
    steps = np.ones(T)
    out = DeviceArray((T, m, n), np.float32)
    dp, dv = DeviceArray.from_host(p), DeviceArray.from_host(v)
    _lib.check(lib.psh_semilag_dev(dp.ptr, dv.ptr, m, n, steps.ctypes.data, T, 1, 1, NAN, None, 0, out.ptr), "semilag_dev")
    return _host(out)


def _semilag_host(lib, p, v, T=3):
    m, n = p.shape
    steps, out, status = np.ones(T), np.empty((T, m, n), np.float32), ctypes.c_int(0)
    _lib.check(lib.psh_semilag_host(p.ctypes.data, v.ctypes.data, m, n, steps.ctypes.data, T, 1, 1, NAN, None, None,
                                    out.ctypes.data, 0, ctypes.byref(status)), "semilag_host")
    return out


def cycle(lib, inp):
    from pysteps_amd.motion import get_method, lucaskanade as lk

    res = {}
    p, v = inp["sl", 72, 104]
    res["sl_72x104"] = _semilag_dev(lib, p, v)
    res["sl_72x104_again"] = _semilag_dev(lib, p, v)  # same step factors: the cached device copy is used
    res["sl_64x96"] = _semilag_dev(lib, *inp["sl", 64, 96])  # a second order table
    _lib.check(lib.psh_set_option(b"trim_cache", 0))
    res["sl_host_first"] = _semilag_host(lib, p, v)
    _lib.check(lib.psh_set_option(b"trim_cache", 0))  # must leave the download stream alone
    res["sl_host_after_trim"] = _semilag_host(lib, p, v)

    res["lk_dense"] = np.array(get_method("LK")(inp["lk"]), copy=True)
    prep = lk.PreparedFrame(DeviceArray.from_host(inp["corner"], dtype=np.float32), 3, 5, True)
    res["lk_corners"] = lk.finish_corners(lk.launch_corners(prep))
    del prep

    for (m, n) in ((64, 64), (17, 31)):
        x = DeviceArray.from_host(inp["fft", (m, n)])
        spec = DeviceArray((m, n // 2 + 1), np.complex128)
        back = DeviceArray((m, n), np.float64)
        _lib.check(lib.psh_fft_rfft2_dev(x.ptr, m, n, spec.ptr), "rfft2")
        _lib.check(lib.psh_fft_irfft2_dev(spec.ptr, m, n, back.ptr), "irfft2")
        res["fft_%dx%d" % (m, n)], res["ifft_%dx%d" % (m, n)] = _host(spec), _host(back)

    field, thr, kr, r = inp["mask"]
    out, x = DeviceArray(field.shape, np.float64), DeviceArray.from_host(field)
    _lib.check(lib.psh_steps_incremental_mask_dev(x.ptr, field.shape[0], field.shape[1], thr,
                                                  kr.ctypes.data_as(ctypes.c_void_p), 3, 3, r, out.ptr), "mask")
    res["mask"] = _host(out)

    initial, target = inp["pm"]
    out, x, spec = DeviceArray((initial.size,), np.float64), DeviceArray.from_host(initial), DeviceArray.from_host(target)
    _lib.check(lib.psh_probmatch_dev(x.ptr, spec.ptr, initial.size, out.ptr), "probmatch")
    res["probmatch"] = _host(out).reshape(initial.shape)
    del out, x, spec, back
    gc.collect()
    return res


def check_against_oracles(inp, res):
    """cycle 1 against what the operation's own test compares with, at that test's bar"""
    from conftest import nan_mismatch, rel_l2
    from oracle import build_ref, lk_opencv as olk, probmatch as opm, semilag_cport as ocl

    with open(os.path.join(ROOT, "tests", "golden", "sl_seen_r05.json")) as fh:
        seen = max(v["rel_l2"] for v in json.load(fh)["seen"].values() if "rel_l2" in v)
    bar = min(max(5.0 * seen, 5e-7), 1e-4)  # tests/test_semilag_gpu.py _bar() for a test it has no record of
    for m, n in ((72, 104), (64, 96)):
        want = ocl.extrapolate(*inp["sl", m, n], 3, n_iter=1)
        got = res["sl_%dx%d" % (m, n)]
        err = rel_l2(got, want)
        print("semilag %dx%d rel-L2 %.3g (bar %.3g)" % (m, n, err, bar))
        assert nan_mismatch(got, want) == 0 and err < bar, (m, n, err)
    for key in ("sl_72x104_again", "sl_host_first", "sl_host_after_trim"):
        assert np.array_equal(res[key], res["sl_72x104"], equal_nan=True), key

    want = olk.dense_lucaskanade(inp["lk"])
    err = rel_l2(res["lk_dense"], want)
    print("dense LK rel-L2 %.3g (bar 1e-3)" % err)
    assert res["lk_dense"].shape == want.shape and err < 1e-3, err
    img = inp["corner"]
    valid = np.isfinite(img)
    want = olk.shitomasi_detection(olk.morph_opening(img, valid, img[valid].min()), valid)
    assert len(want) > 0 and np.array_equal(res["lk_corners"], want)

    def c(a, b):
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))

    for shape in ((64, 64), (17, 31)):
        x, tag = inp["fft", shape], "%dx%d" % shape
        errs = c(res["fft_" + tag], np.fft.rfft2(x)), c(res["ifft_" + tag], x)
        print("fft %s: %.3g forward, %.3g round trip (bar 1e-12)" % ((tag,) + errs))
        assert max(errs) < 1e-12, (shape, errs)

    assert build_ref.available(), "oracle/_ref is not built"
    build_ref.activate()
    from pysteps.nowcasts.utils import compute_dilated_mask as ref_mask

    field, thr, kr, r = inp["mask"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = ref_mask(field >= thr, kr, r)
    assert np.array_equal(res["mask"], want, equal_nan=True)

    want = opm.nonparam_match_empirical_cdf(*inp["pm"])
    assert np.array_equal(res["probmatch"], want)


def hbm_free(lib):
    free = ctypes.c_size_t(0)
    _lib.check(lib.psh_device_info(None, None, None, ctypes.byref(free), None, 0), "device_info")
    return int(free.value)


def main():
    lib = _lib.load()
    inp = _inputs()
    device = _lib.default_device()
    first, free, held = None, [], None
    for number in (1, 2, 3):
        rc = lib.psh_init(device)
        assert rc == 0, ("psh_init", number, rc, _lib.last_error())
        _lib._initialised = True
        free.append(hbm_free(lib))
        print("cycle %d: hbm_free %d after psh_init" % (number, free[-1]), flush=True)
        if held is not None:  # blocks that went with the shutdown: PSH_EINVAL (unknown pointer), nothing is freed twice
            codes = lib.psh_free(held[0]), lib.psh_host_free(held[1])
            print("held across the shutdown: psh_free -> %d, psh_host_free -> %d" % codes)
            assert codes == (_lib.PSH_EINVAL, _lib.PSH_EINVAL), codes
            held = None
        res = cycle(lib, inp)
        if first is None:
            first = res
            check_against_oracles(inp, res)
        else:
            assert sorted(res) == sorted(first)
            bad = []
            for key in sorted(res):
                a, b = first[key], res[key]
                if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
                    where = np.flatnonzero(a.ravel().view(np.uint8) != b.ravel().view(np.uint8)) if a.shape == b.shape else []
                    print("cycle %d: %s differs from cycle 1 in %d of %d bytes, first at byte %s" %
                          (number, key, len(where), a.nbytes, where[:4]), flush=True)
                    bad.append(key)
            assert not bad, (number, bad)
        if number == 2:
            dev, host = ctypes.c_void_p(), ctypes.c_void_p()
            _lib.check(lib.psh_malloc(ctypes.byref(dev), 3 << 20), "psh_malloc")
            _lib.check(lib.psh_host_alloc(ctypes.byref(host), 3 << 20), "psh_host_alloc")
            held = (dev.value, host.value)
        gc.collect()
        rc = lib.psh_shutdown()
        assert rc == 0, ("psh_shutdown", number, rc, _lib.last_error())
        assert lib.psh_free(None) == 0 and lib.psh_sync() == _lib.PSH_ENOTINIT
    # after the last shutdown every entry point answers what it answers before the first psh_init (in-process: none of
    # these calls gets as far as the device, and a process that has opened the GPU does not fork)
    from helpers import entry_points
    from test_entry_points_cpu import EXPECTED

    got = {name: entry_points.call(lib, name) for name in entry_points.names()}
    wrong = {name: (got[name], EXPECTED[name]) for name in EXPECTED if got.get(name) != EXPECTED[name]}
    assert sorted(got) == sorted(EXPECTED) and not wrong, wrong
    print("after the last shutdown: %d entry points answer as before psh_init" % len(got))
    print("hbm_free after each psh_init: %s" % free)
    print("shutdown cycles: ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
