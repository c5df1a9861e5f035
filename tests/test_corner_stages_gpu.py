"""The Shi-Tomasi front end of dense Lucas-Kanade, stage by stage, against oracle/lk_opencv.py: the response plane
(lk_corner_response_cols), its maximum (lk_max_final), the candidate set (lk_corner_select), the accepted corners and
the fused pass (lk_corner_response_nms).  Everything is integer or exactly rounded float32 work: every comparison is
bit for bit.  The entry points are fed directly: ``feature_u8`` is an image of tests/helpers/corner_cases.py, ``clean``
a plane that only carries the NaN pattern, ``stats`` a block with the NaN count set."""

import ctypes

import numpy as np
import pytest

from helpers import corner_cases as cc

pytestmark = pytest.mark.gpu

GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    """The library, the device array type and the statistics indices of the banded estimate."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.motion import banded

    class Dev:
        pass

    d = Dev()
    d.lib, d.check, d.Array, d.banded = _lib.lib(), _lib.check, DeviceArray, banded
    d.n_stats, d.nan_count, d.eig_max = banded._N_STATS, banded._NAN_COUNT, banded._EIG_MAX
    return d


class Stage:
    """One image on the device with the planes the corner entry points take."""

    def __init__(self, dev, u8, nan_kind="none", buffer_mask=5, mask=None):
        from oracle import lk_opencv as olk

        self.dev, self.u8 = dev, np.ascontiguousarray(u8)
        self.m, self.n = u8.shape
        self.buffer_mask = int(buffer_mask)
        self.mask = cc.nan_mask(nan_kind, self.m, self.n) if mask is None else mask
        self.allowed = ~olk.dilate_mask(self.mask, self.buffer_mask)
        self.u8_dev = dev.Array.from_host(self.u8)
        self.clean_dev = dev.Array.from_host(cc.clean_plane(self.mask))
        stats = np.zeros(dev.n_stats, np.float32)
        stats[dev.nan_count] = self.mask.sum()
        self.stats_dev = dev.Array.from_host(stats)
        self.eig_dev = dev.Array((self.m, self.n), np.float32).fill_bytes(0xFF)  # NaN until written

    def whole(self):
        return (0, self.m, 0, self.m)

    def response(self, block_size, band=None):
        """-> (plane, statistics) after psh_lk_band_response_dev over ``band`` = (e0, e1, r0, r1)."""
        e0, e1, r0, r1 = band or self.whole()
        d = self.dev
        d.check(d.lib.psh_lk_band_response_dev(self.u8_dev.ptr, self.clean_dev.ptr, self.m, self.n, e0, e1, r0, r1,
                                               int(block_size), self.buffer_mask, self.stats_dev.ptr, self.eig_dev.ptr),
                "band_response")
        return self.eig_dev.to_host().copy(), self.stats_dev.to_host().copy()

    def select(self, quality, cap=None, band=None, spare=0):
        """-> (count, key buffer of cap + spare words) after psh_lk_band_select_dev on the plane of response()."""
        e0, e1, r0, r1 = band or self.whole()
        d = self.dev
        cap = max(self.m * self.n, 1) if cap is None else cap
        keys = d.Array.from_host(np.full(cap + spare, GUARD, np.uint64))
        count = d.Array.from_host(np.full(1, -1, np.int32))
        d.check(d.lib.psh_lk_band_select_dev(self.eig_dev.ptr, self.clean_dev.ptr, self.m, self.n, e0, e1, r0, r1,
                                             self.buffer_mask, float(quality), self.stats_dev.ptr, keys.ptr, int(cap),
                                             count.ptr), "band_select")
        return int(count.to_host()[0]), keys.to_host().copy()

    def corners(self, block_size, max_corners, min_distance, quality=0.01):
        d = self.dev
        pts = np.empty((int(max_corners), 2), np.float32)
        count = ctypes.c_int(0)
        d.check(d.lib.psh_lk_corners_dev(self.u8_dev.ptr, self.clean_dev.ptr, self.stats_dev.ptr, self.m, self.n,
                                         int(block_size), self.buffer_mask, float(quality), float(min_distance),
                                         int(max_corners), pts.ctypes.data, ctypes.byref(count)), "lk_corners")
        return pts[: count.value].copy()


def _max_bits(eig, allowed, rows=slice(None)):
    """max(0, maximum over the allowed pixels of the rows) as float32 bits."""
    vals = eig[rows][allowed[rows]]
    return _bits(np.float32(max(np.float32(0), vals.max())) if vals.size else np.float32(0))


# ---- (a) the response plane ------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_size", cc.BLOCK_SIZES)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_response_plane(dev, shape, block_size):
    """Every pixel of the plane, as bits: the borders (mirrored walk, few_rows route), shapes whose edges lie on, one
    past and below the strips of crn_cols(BS) columns and the bands of 32 rows, the heights whose preload used to
    leave the image."""
    from oracle import lk_opencv as olk

    m, n = shape
    for family in ("noise", "two_level", "ramp_impulse"):
        u8 = cc.image(family, m, n)
        stage = Stage(dev, u8)
        got, stats = stage.response(block_size)
        want = olk.corner_min_eigenval(u8, block_size)
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, (family, len(bad), bad[:5].tolist())
        assert _bits(stats[dev.eig_max]) == _max_bits(want, stage.allowed), family


# ---- (b) the maximum -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buffer_mask", [0, 1, 5, 6])
@pytest.mark.parametrize("nan_kind", cc.NAN_KINDS)
def test_maximum_over_the_allowed_pixels(dev, nan_kind, buffer_mask):
    """stats[EIG_MAX] = max(0, max over pixels outside the dilated NaN mask); the even buffer exercises the
    size // 2 anchor of the dilation."""
    from oracle import lk_opencv as olk

    for m, n in ((40, 130), (17, 63), (9, 57), (129, 117)):
        for family, block_size in (("noise", 1), ("noise", 5), ("ramp_impulse", 3), ("two_level", 7)):
            u8 = cc.image(family, m, n)
            stage = Stage(dev, u8, nan_kind, buffer_mask)
            _, stats = stage.response(block_size)
            want = olk.corner_min_eigenval(u8, block_size)
            assert _bits(stats[dev.eig_max]) == _max_bits(want, stage.allowed), (m, n, family, block_size)


@pytest.mark.parametrize("buffer_mask", [0, 1, 5, 6])
@pytest.mark.parametrize("block_size", cc.BLOCK_SIZES)
def test_maximum_under_the_mask_does_not_count(dev, block_size, buffer_mask):
    """A missing pixel whose buffer covers the strongest response: the maximum is the runner-up's.  For the even
    buffer the pixel sits where only the longer side of the 6 x 6 window (anchor 3: rows and columns -3 .. +2 as seen
    from the judged pixel) reaches the response."""
    from oracle import lk_opencv as olk

    m, n = 40, 130
    u8 = cc.image("noise", m, n)
    want = olk.corner_min_eigenval(u8, block_size)
    y, x = np.unravel_index(np.argmax(want), want.shape)
    reach = buffer_mask // 2
    mask = np.zeros((m, n), bool)
    mask[max(y - reach, 0), max(x - reach, 0)] = True
    stage = Stage(dev, u8, buffer_mask=buffer_mask, mask=mask)
    assert not stage.allowed[y, x] or (buffer_mask and (y < reach or x < reach))
    _, stats = stage.response(block_size)
    assert _bits(stats[dev.eig_max]) == _max_bits(want, stage.allowed)
    if not stage.allowed[y, x] and np.count_nonzero(want == want[y, x]) == 1:  # (block_size 1: the maximum is tied)
        assert stats[dev.eig_max] < want[y, x]


# ---- (c) the candidate set -------------------------------------------------------------------------------------
QUALITIES = (0.01, 0.5, 1.0, 0.0)
FEW_SHAPES = [(1, 1), (3, 70), (7, 9), (11, 57), (16, 59), (33, 61), (34, 63), (17, 63), (65, 249), (40, 130), (129, 117)]
CANDIDATE_CASES = [("noise", s) for s in cc.SHAPES]
CANDIDATE_CASES += [(f, s) for f in ("period4", "blocks8", "ramp_impulse", "rain") for s in FEW_SHAPES]
CANDIDATE_CASES += [("flat", (7, 9)), ("flat", (40, 130))]


@pytest.mark.parametrize("family,shape", CANDIDATE_CASES, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_candidate_set(dev, family, shape):
    """Count and keys of psh_lk_band_select_dev on the plane of (a) against the oracle's candidate stage, for every
    block size and quality level; the NaN mask changes with both, so that each kind meets each of them."""
    from oracle import lk_opencv as olk

    m, n = shape
    u8 = cc.image(family, m, n)
    stages = {kind: Stage(dev, u8, kind) for kind in cc.NAN_KINDS}
    for i, block_size in enumerate(cc.BLOCK_SIZES):
        for j, quality in enumerate(QUALITIES):
            nan_kind = cc.NAN_KINDS[(i + j) % len(cc.NAN_KINDS)]
            stage = stages[nan_kind]
            stage.response(block_size)
            count, keys = stage.select(quality)
            eig, eig_max, want = olk.corner_candidates(u8, stage.allowed, quality, block_size)
            where = (block_size, quality, nan_kind)
            if want.size and eig_max <= 0:
                # no positive response among the allowed pixels: OpenCV's threshold is then negative or zero and its
                # list may hold negative responses; the device's maximum is clamped at zero and it takes none
                want = want[:0]
            assert count == want.size, (where, count, want.size)
            assert np.array_equal(np.sort(keys[:count]), np.sort(want)), where
            assert np.all(keys[count:] == 0), where  # the rest of the buffer is cleared
            if family == "flat":
                assert count == 0 and np.all(eig == 0)
            if quality == 1.0:
                assert count == 0


# ---- (d) a key buffer smaller than the candidate list ----------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 63), (40, 130), (129, 117)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", ["noise", "period4"])
def test_small_cap(dev, family, shape):
    from oracle import lk_opencv as olk

    m, n = shape
    u8 = cc.image(family, m, n)
    for block_size in (3, 5):
        stage = Stage(dev, u8)
        stage.response(block_size)
        want = olk.corner_candidates(u8, stage.allowed, 0.01, block_size)[2]
        cap = want.size // 3
        assert cap >= 4
        count, keys = stage.select(0.01, cap=cap, spare=257)
        assert count == want.size                       # the count is the total
        assert np.all(keys[cap:] == GUARD)              # nothing behind cap was written
        assert np.unique(keys[:cap]).size == cap and np.isin(keys[:cap], want).all()


# ---- (e) row bands ---------------------------------------------------------------------------------------------
BAND_EDGES = (0, 16, 33, 64, 129)


def _bands(m, block_size):
    """(e0, e1, r0, r1) per band: the extension is the least the kernels need (block_size // 2 + 2 rows: the
    response of the rows next to the own ones and their stencils) for every other band, five rows more otherwise."""
    need = block_size // 2 + 2
    out = []
    for k, (r0, r1) in enumerate(zip(BAND_EDGES[:-1], BAND_EDGES[1:])):
        ext = need + (5 if k % 2 else 0)
        out.append((max(0, r0 - ext), min(m, r1 + ext), r0, r1))
    return out


@pytest.mark.parametrize("nan_kind", ["none", "corner_block"])
@pytest.mark.parametrize("family", ["noise", "period4"])
@pytest.mark.parametrize("block_size", cc.BLOCK_SIZES)
def test_row_bands(dev, block_size, family, nan_kind):
    """Bands with inner edges at 16, 33 and 64 of a 129 x 117 image: the own rows of every band's plane are the
    whole-frame rows, EIG_MAX is the maximum over the own rows, and the keys the banded estimate gathers
    (banded._corner_candidates: response, maximum exchanged on the host, selection) are the whole-frame set."""
    from oracle import lk_opencv as olk

    m, n = 129, 117
    assert BAND_EDGES[-1] == m
    u8 = cc.image(family, m, n)
    whole = Stage(dev, u8, nan_kind)
    eig, eig_max, want = olk.corner_candidates(u8, whole.allowed, 0.01, block_size)
    frames = []
    for band in _bands(m, block_size):
        e0, e1, r0, r1 = band
        assert (e0 == 0 or r0 - e0 >= block_size // 2 + 2) and (e1 == m or e1 - r1 >= block_size // 2 + 2)
        stage = Stage(dev, u8, nan_kind)
        got, stats = stage.response(block_size, band)
        assert np.array_equal(_bits(got[r0:r1]), _bits(eig[r0:r1])), band
        assert _bits(stats[dev.eig_max]) == _max_bits(eig, whole.allowed, slice(r0, r1)), band
        # the banded estimate's own candidate stage on the same planes
        bf = dev.banded._BandFrame(stage.clean_dev, (r0, r1, e0, e1), 0, stage.buffer_mask, True)
        bf.clean, bf.feature_u8 = stage.clean_dev, stage.u8_dev
        bf.stats = dev.Array.from_host(np.where(np.arange(dev.n_stats) == dev.nan_count, whole.mask.sum(), 0)
                                       .astype(np.float32))
        bf.keep = stage
        frames.append(bf)
    parts = dev.banded.run_virtual([dev.banded._corner_candidates(bf, block_size, 0.01) for bf in frames])
    for bf, part in zip(frames, parts):
        assert _bits(bf.global_stats[dev.eig_max]) == _max_bits(eig, whole.allowed)  # the exchanged maximum
        rows = (part & np.uint64(0xFFFFFFFF)).astype(np.int64) // n
        assert np.all((rows >= bf.rows[0]) & (rows < bf.rows[1]))
    union = np.concatenate(parts)
    assert union.size == want.size and np.array_equal(np.sort(union), np.sort(want))


# ---- (f) accepted corners on hard images -----------------------------------------------------------------------
@pytest.mark.parametrize("block_size", cc.BLOCK_SIZES)
@pytest.mark.parametrize("shape", cc.HARD_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", ["noise", "period4", "blocks8"])
def test_corners_on_hard_images(dev, family, shape, block_size):
    """psh_lk_corners_dev against goodFeaturesToTrack: the same points in the same order, on images full of tied
    responses; max_corners = 3000 takes the route that orders the candidates on the host."""
    from oracle import lk_opencv as olk

    m, n = shape
    u8 = cc.image(family, m, n)
    stage = Stage(dev, u8, "pixel")
    for max_corners, min_distance in ((1000, 10), (3000, 0), (50, 3.5)):
        want = olk.good_features_to_track(u8, stage.allowed, max_corners, 0.01, min_distance, block_size)
        got = stage.corners(block_size, max_corners, min_distance)
        # (period4 under a 1 x 1 block: lambda_min of a rank-one matrix, rounding noise at most - no candidates)
        assert len(want) > 10 or (family == "period4" and block_size == 1 and len(want) == 0)
        assert got.shape == want.shape and np.array_equal(got, want), (max_corners, min_distance)


# ---- (g) the fused pass ----------------------------------------------------------------------------------------
def _frame_pair(family, m, n):
    """Two float32 frames with the integer values 0 .. 255 of a family's image, both ends present below the rows the
    feature rendering leaves out of its range, the second frame one pixel to the right."""
    img = cc.image(family, m, n).astype(np.float32)
    img[m // 2, 1], img[m // 2, 3] = 0, 255
    if family == "rain":
        img[m // 3: m // 3 + max(m // 5, 2), n // 2: n // 2 + n // 6] = np.nan
    return np.stack([img, np.roll(img, 1, axis=1)])


@pytest.mark.parametrize("block_size", cc.BLOCK_SIZES)
@pytest.mark.parametrize("shape", [(40, 130), (129, 117), (11, 57)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", ["noise", "period4", "rain"])
def test_fused_pass_gives_the_same_vectors(dev, family, shape, block_size):
    """psh_set_option("lk_fused_nms", 1): response, 3x3 maxima and compaction in one pass, for resident float32
    frames.  The sparse vectors are identical with and without it.  Where the images can fill a wave's 64 slots -
    period4 at every shape, noise from 40 x 130 on (tests/test_corner_stages_cpu.py) - the device's own rendering of
    frame 0 is shown to put more than 64 candidates into one tile of the fused geometry first: the spill path behind
    the fixed slots was needed.  (Rain fields hold a few maxima per tile; they bring the NaN block.)  No opening: it
    would flatten period4."""
    from oracle import lk_opencv as olk
    from pysteps_amd.motion import lucaskanade as lk

    m, n = shape
    frames = _frame_pair(family, m, n)
    assert frames[0][np.isfinite(frames[0])].min() == 0 and frames[0][np.isfinite(frames[0])].max() == 255
    resident = dev.Array.from_host(frames)
    prep = lk.PreparedFrame(resident.view(0), 0, 5, True)
    u8 = prep.feature_u8.to_host().copy()
    allowed = ~olk.dilate_mask(~np.isfinite(frames[0]), 5)
    keys = olk.corner_candidates(u8, allowed, 0.01, block_size)[2]
    fullest = cc.tile_counts(keys, m, n, *cc.fused_tile(block_size)).max() if keys.size else 0
    if (family == "period4" and block_size > 1) or (family == "noise" and m >= 40):
        assert fullest > cc.NMS_KEYS, fullest
    results = []
    try:
        for fused in (0, 1):
            dev.check(dev.lib.psh_set_option(b"lk_fused_nms", fused))
            results.append(lk.dense_lucaskanade(resident, dense=False, size_opening=0,
                                                fd_kwargs={"block_size": block_size}))
    finally:
        dev.check(dev.lib.psh_set_option(b"lk_fused_nms", 0))
    (xy0, uv0), (xy1, uv1) = results
    assert xy0.shape == xy1.shape and np.array_equal(xy0, xy1) and np.array_equal(uv0, uv1)
    if keys.size and family != "period4":
        assert len(xy0) > 0  # (every window of period4 looks the same: whatever the tracker makes of it)
