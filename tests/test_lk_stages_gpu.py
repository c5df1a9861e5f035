"""The stages between the uint8 frames and the tracked points of dense Lucas-Kanade, each against the OpenCV
restatement (oracle/lk_opencv.py): Gaussian pyramid levels and the Scharr gradient image bit for bit through the
read-out of the pyramid set, ONE tracker iteration within an error bound derived from its exact integer sums
(``first_step``), and the whole tracker on frames of saturated contrast.  All frames are uint8, built on the host
(tests/helpers/lk_stage_cases.py); the conditions on the cases are checked in tests/test_lk_stages_cpu.py."""

import ctypes

import numpy as np
import pytest

from helpers import lk_stage_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lkmod():
    from pysteps_amd.motion import lucaskanade

    return lucaskanade


def _check_levels(pair, a, b, win, max_level, deriv):
    from oracle import lk_opencv as olk

    want_i, want_j = olk.build_pyramid(a, win, max_level), olk.build_pyramid(b, win, max_level)
    assert pair.top == len(want_i) - 1
    for l, (wi, wj) in enumerate(zip(want_i, want_j)):
        gi, gj, gd = pair.level(l)
        assert gi.shape == wi.shape and gj.shape == wj.shape, (l, gi.shape, wi.shape)
        bad_i, bad_j = np.argwhere(gi != wi), np.argwhere(gj != wj)
        assert not len(bad_i) and not len(bad_j), "level %d: %d + %d bytes differ, first at %s" % (
            l, len(bad_i), len(bad_j), (bad_i[0] if len(bad_i) else bad_j[0]))
        if deriv:
            ix, iy = olk.scharr_deriv(wi)
            assert gd.dtype == np.int16 and gd.shape == wi.shape + (2,)
            bad = np.argwhere((gd[..., 0] != ix) | (gd[..., 1] != iy))
            assert not len(bad), "level %d: %d gradients differ, first at %s" % (l, len(bad), bad[0])
        else:
            assert gd is None


PYR_RUNS = [(c, "binary") for c in C.PYR_CASES] + [(c, "smooth") for c in C.PYR_SMOOTH]


@pytest.mark.parametrize("case,family", PYR_RUNS, ids=["%dx%d-%s" % (c[0], c[1], f) for c, f in PYR_RUNS])
def test_pyramid_levels_bit_for_bit(lkmod, case, family):
    m, n, win, max_level = case
    a, b = C.FAMILIES[family](m, n, 3 * m + n), C.FAMILIES[family](m, n, 3 * m + n + 1)
    pair = lkmod.PyramidPair(C.U8Frame(a), C.U8Frame(b), win, max_level)
    _check_levels(pair, a, b, win, max_level, deriv=False)
    pair.close()


@pytest.mark.parametrize("lead", [1, 3])
def test_pyramid_from_an_unaligned_level0_pointer(lkmod, lead):
    """Rows of a multiple of four bytes, but the frame starts ``lead`` bytes into its allocation: level 1 has to
    be assembled from bytes, the levels above take the fast route again."""
    m, n, win, max_level = C.PYR_UNALIGNED
    a, b = C.binary(m, n, 11), C.binary(m, n, 12)
    fa, fb = C.U8Frame(a, lead), C.U8Frame(b, lead)
    assert fa.ptr % 4 == lead and fb.ptr % 4 == lead
    pair = lkmod.PyramidPair(fa, fb, win, max_level)
    _check_levels(pair, a, b, win, max_level, deriv=False)
    pair.close()


SCHARR_RUNS = [(w, s, f) for w in C.SCHARR_WINDOWS for s in C.SCHARR_SHAPES for f in ("binary", "edges")]


@pytest.mark.parametrize("win,shape,family", SCHARR_RUNS,
                         ids=["%dx%d-%dx%d-%s" % (w + s + (f,)) for w, s, f in SCHARR_RUNS])
def test_gradient_image_bit_for_bit(lkmod, win, shape, family):
    m, n = shape
    a, b = C.FAMILIES[family](m, n, m + n), C.FAMILIES[family](m, n, m + n + 1)
    pair = lkmod.PyramidPair(C.U8Frame(a), C.U8Frame(b), win, 3)
    _check_levels(pair, a, b, win, 3, deriv=True)
    pair.close()


def test_no_gradient_image_up_to_61_columns_and_read_out_arguments(lkmod):
    from pysteps_amd import _lib

    lib = _lib.lib()
    a, b = C.binary(130, 131, 1), C.binary(130, 131, 2)
    pair = lkmod.PyramidPair(C.U8Frame(a), C.U8Frame(b), (61, 20), 3)
    assert pair.top == 1
    assert all(pair.level(l)[2] is None for l in range(pair.top + 1))
    # refused requests leave the buffer alone
    buf = np.full(130 * 131 * 4, 0xA5, np.uint8)
    rows = ctypes.c_int(-1)
    for level, plane, nbytes in ((2, 0, 33 * 33), (-1, 0, 130 * 131), (0, 0, 130 * 131 - 1), (0, 1, 130 * 131 + 1),
                                 (0, 2, 130 * 131 * 4), (0, 3, 130 * 131)):
        assert lib.psh_lk_pyramids_read(pair._h, level, plane, buf.ctypes.data, nbytes) == _lib.PSH_EINVAL
    assert lib.psh_lk_pyramids_read(None, 0, 0, buf.ctypes.data, 130 * 131) == _lib.PSH_EINVAL
    assert lib.psh_lk_pyramids_shape(pair._h, 2, ctypes.byref(rows), None, None, None) == _lib.PSH_EINVAL
    assert lib.psh_lk_pyramids_shape(None, 0, ctypes.byref(rows), None, None, None) == _lib.PSH_EINVAL
    assert (buf == 0xA5).all() and rows.value == -1
    pair.close()


@pytest.mark.parametrize("win,family", C.STEP_CASES, ids=[C.case_id(*c) for c in C.STEP_CASES])
def test_one_tracker_step_within_the_derived_bound(lkmod, win, family):
    """nr_levels = 0 and criteria (COUNT | EPS, 1, 0): the tracker leaves p + d after exactly one iteration, d a
    fixed float32 expression of five exact integer sums.  |got - want| <= 2 * bound per component and point, the
    bound from ``oracle.lk_opencv.first_step`` (float32 roundings of either side, fused or not); status equal
    for every point; a point that takes no step comes back bit for bit."""
    a, b, pts = C.step_case(win, family)
    res = C.step_oracle(win, family)
    pair = lkmod.PyramidPair(C.U8Frame(a), C.U8Frame(b), win, 0)
    got, gst = pair.track(pts, criteria=(3, 1, 0.0))
    pair.close()
    assert np.array_equal(gst, res["status"]), np.flatnonzero(gst != res["status"])
    still = ~res["stepped"]
    assert np.array_equal(got[still].view(np.uint32), pts[still].view(np.uint32))
    keep = C.compared(res)
    err = np.abs(got.astype(np.float64) - res["next"].astype(np.float64))
    ratio = err[keep] / res["bound"][keep]
    print("one step %s: %d points, largest |got - want| / bound %.3f, largest |got - want| %.3e px"
          % (C.case_id(win, family), keep.sum(), ratio.max(), err[keep].max()))
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert (ratio <= 2.0).all(), (pts[keep][worst[0]], got[keep][worst[0]], res["next"][keep][worst[0]])


@pytest.mark.parametrize("win,family", C.FULL_CASES, ids=["%dx%d-%s" % (w + (f,)) for w, f in C.FULL_CASES])
def test_full_tracking_on_saturated_contrast(lkmod, win, family):
    """The whole pyramidal tracker where every range argument of the kernels is at its limit."""
    from oracle import lk_opencv as olk

    a, b, pts = C.full_case(win, family)
    want, wst = olk.calc_optical_flow_pyr_lk(a, b, pts, win=win, max_level=2)
    got, gst = lkmod.track_points(C.U8Frame(a), C.U8Frame(b), pts, winsize=win, nr_levels=2)
    assert len(pts) == 30 and wst.sum() >= 15
    assert np.array_equal(gst, wst), np.flatnonzero(gst != wst)
    print("full %dx%d %s: %d tracked, largest difference %.3e px" % (win + (family, wst.sum(), np.abs(got[wst] - want[wst]).max())))
    assert np.abs(got[wst] - want[wst]).max() < 1e-2
