"""The cases and the oracle of tests/test_lk_stages_gpu.py, checked without a device: the pyramid shapes reach
every route of lk_pyrdown, ``first_step`` is the tracker restatement's first iteration bit for bit, its error bound
holds against float64, the points that are compared are enough and clear of every threshold, and the frames fill
the integer ranges the tracker kernels rely on."""

import numpy as np
import pytest

from helpers import lk_stage_cases as C

STEP_IDS = [C.case_id(*c) for c in C.STEP_CASES]


def test_route_census_lists_every_route():
    seen = {}
    for case in C.PYR_CASES:
        for r in C.case_routes(*case):
            seen.setdefault(r, []).append(case[:2])
    assert sorted(seen) == sorted(C.ROUTES), sorted(set(C.ROUTES) - set(seen))
    # the shapes that are there for one route each
    assert {"fast", "border_bytes", "store_dword"} <= C.case_routes(256, 256, (21, 21), 3)
    assert "unaligned_bytes" in C.case_routes(130, 131, (9, 7), 3) and "unaligned_bytes" in C.case_routes(257, 255, (9, 7), 3)
    assert "small_reflect" in C.case_routes(40, 23, (5, 5), 3)
    assert {"store_dword", "store_bytes"} <= C.case_routes(96, 264, (9, 7), 3)
    assert "half2_skipped" in C.pyrdown_routes(66, 96, 33, 48) and "half2_cut" in C.pyrdown_routes(90, 96, 45, 48)
    assert "blocks_x" in C.case_routes(48, 1100, (5, 5), 3)
    # a source of aligned rows behind an unaligned pointer loses the fast route at level 0 only
    assert "fast" not in C.pyrdown_routes(64, 128, 32, 64, src_aligned=False)
    assert {"fast", "unaligned_bytes"} <= C.case_routes(*C.PYR_UNALIGNED, lead=1)
    # every case has at least three levels
    assert all(len(C.level_shapes(*case)) >= 3 for case in C.PYR_CASES)


def test_instantiations_named_in_the_ids():
    want = {(5, 5): ("rows", 8), (9, 7): ("rows", 8), (21, 21): ("rows", 8), (50, 50): ("rows", 13),
            (61, 33): ("rows", 13), (15, 61): ("rows", 16), (62, 20): ("gather", 10), (63, 40): ("gather", 10),
            (64, 64): ("gather", 16), (64, 3): ("gather", 4)}
    assert {w: C.instantiation(w) for w in C.STEP_WINDOWS} == want


@pytest.mark.parametrize("win,family", C.STEP_CASES, ids=STEP_IDS)
def test_first_step_is_the_restatement_and_its_bound_holds(win, family):
    from oracle import lk_opencv as olk

    a, b, pts = C.step_case(win, family)
    res = C.step_oracle(win, family)
    want, wst = olk.calc_optical_flow_pyr_lk(a, b, pts, win=win, max_level=0, max_count=1, epsilon=0.0)
    assert np.array_equal(res["next"].view(np.uint32), want.view(np.uint32)) and np.array_equal(res["status"], wst)
    # no step: the point comes back as it went in
    assert np.array_equal(res["next"][~res["stepped"]], pts[~res["stepped"]])
    # the float32 evaluation against float64 from the same exact sums
    s = res["stepped"]
    err = np.abs(res["next"].astype(np.float64) - (pts.astype(np.float64) + res["d64"]))
    assert (err[s] <= res["bound"][s]).all(), (err[s] / res["bound"][s]).max()
    # the bound is worth having: far below the 1e-2 px of the whole-tracker tests
    keep = C.compared(res)
    assert res["bound"][keep].max() < 1e-4


@pytest.mark.parametrize("win,family", C.STEP_CASES, ids=STEP_IDS)
def test_enough_points_are_compared_and_none_sits_at_a_threshold(win, family):
    res = C.step_oracle(win, family)
    _, _, pts = C.step_case(win, family)
    keep = C.compared(res)
    assert keep.sum() >= (20 if family != "planes" else 15)
    assert (~keep).sum() <= 0.25 * len(pts)
    # whatever is compared, and every status that is asserted, is clear of the decisions' float noise; a point
    # near a threshold is not compared and counts against the 25 % above
    assert (res["margin"][keep] >= C.MIN_MARGIN).all()
    # status: the rejected ones are rejected by a wide margin too (they are asserted on the device)
    assert (res["margin"] >= C.MIN_MARGIN).all()
    if family != "planes":
        st = res["status"]
        beyond, flat = slice(38, 42), 42
        assert not st[beyond].any() and not st[flat] and not res["stepped"][flat]
        assert st[:14].sum() >= 12 and st[14:34].sum() >= 16  # interior; borders, corners, integer / half positions


def _fill(win, family):
    """Largest share of a thread in S11 / S12 / S22 and largest |diff * g| of a sample over the points of a case."""
    res = C.step_oracle(win, family)
    share = prod = 0
    for patches in res["patches"]:
        if patches is None:
            continue
        _, gx, gy, diff = patches
        for v in (gx * gx, np.abs(gx * gy), gy * gy):
            share = max(share, int(C.thread_shares(v, win).max()))
        prod = max(prod, int(np.abs(diff * gx).max()), int(np.abs(diff * gy).max()))
    return share, prod


def test_frames_fill_the_ranges_the_kernels_rely_on():
    """The kernels keep a thread's partial sums in 32 bits and their products on the 24-bit multiplier, and say why:
    |g| <= 16 * 255 and at most 16 samples per thread, so a share of S11 is at most 16 * (16 * 255)^2 = 266 342 400
    (12.4 % of 2^31); |diff| <= 255 * 32, so |diff * g| <= 33 292 800 (49.6 % of 2^26).  No uint8 frame can go
    beyond these two figures, so they - not 2^31 and 2^26 themselves - are what a frame can be asked to reach."""
    share_cap = C.SHARE_SAMPLES * C.GRAD_MAX ** 2
    prod_cap = C.DIFF_MAX * C.GRAD_MAX
    assert share_cap < 2 ** 31 and prod_cap < 2 ** 26
    for win in ((64, 64), (15, 61)):  # 16 samples per thread
        assert C.instantiation(win)[1] == C.SHARE_SAMPLES
        share, prod = _fill(win, "binary")
        print("binary %dx%d: share %.3f, |diff g| %.3f of the caps" % (win[0], win[1], share / share_cap, prod / prod_cap))
        # random 0 / 255 pixels do not line sixteen full-scale gradients up in one thread: the constructed frame does
        share, prod = _fill(win, "planes")
        print("planes %dx%d: share %.3f, |diff g| %.3f of the caps" % (win[0], win[1], share / share_cap, prod / prod_cap))
        assert share >= 0.9 * share_cap and prod >= 0.9 * prod_cap
        assert share <= share_cap and prod <= prod_cap
