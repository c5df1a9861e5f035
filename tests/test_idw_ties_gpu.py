"""The HIP k-NN IDW kernels at EXACTLY equidistant samples, against the exact oracle of tests/helpers/idw_exact.py.

tests/test_idw_gpu.py leaves out every pixel whose k-th and (k+1)-th nearest samples are equidistant and uses
continuous random positions.  The real workload is the opposite: Shi-Tomasi corners sit on integer pixels, declustered
vectors on half integers, the nodes are integers - 1 to 30 % of the pixels have such a tie.  For these inputs the squared
distances are exact in float32 (asserted per case, before anything else), so ties are exact on both sides and NO pixel is
left out of any assertion here.

Per case, bars as in tests/test_idw_gpu.py (float32 arithmetic against a float64 reference: max abs <= 1e-4, relative
L2 < 1e-5):
  A  validity   every pixel equals, for SOME r-subset of its tie set, the exact weighted mean;
  B  the rule   every pixel equals the field of the documented rule: ties go to the lower sample index
                (csrc/idw.hip: add_nearest, idw_small_ring2, TopK);
  C  paths      the two-level kernels (default) and the one-level kernel (idw_variant 1) agree to 1e-5 on all pixels,
                and idwinterp2d (host arrays) is bit-identical to idw_to_device (resident arrays).
Every case also asserts, on the CPU and for the oracle alone, that it has enough DISCRIMINATING tie pixels: pixels
where another valid subset moves the value by more than 10 x the bar, so that B can tell the rule from any other
choice.  The floor is 100; the two one-pixel-wide images have 77 pixels in all, their floor is 40 (more than half of
the image: the samples come in pairs mirrored at the pixel line, so a pair straddles rank k almost everywhere); the
cases with k >= L have no tie set by definition (every sample is a member) and assert that there is none.

Which kernel path a tile takes is not observable; the cases are built from the constants of csrc/idw.hip (supertile
64 x 64 with a list of kSuperCap = 256 samples, fine tile 16 x 8 with kFineCap = 96, a ring of <= 8 undecided samples
ranked pairwise, KMAX instantiations 8 / 20 / 32, kCandCap = 512 in the one-level kernel) and say which path they aim at.

case                        L    pixels  tie pixels  discriminating  largest tie group  samples on a node
int200_48x80_k20           200    3840      603          603               5                 200
int150_64x64_k5            150    4096      455          455               4                 150
int150_64x64_k1            150    4096      354          354               3                 150
int150_64x64_k5_power2     150    4096      455          443               4                 150
lattice8_100x100_k8        169   10000     2641         2641               8                 169
lattice8_100x100_k9        169   10000     3890         3890               8                 169
lattice8_100x100_k20       169   10000     3121         3121               8                 169
lattice8_100x100_k21       169   10000     4261         4261               8                 169
lattice8_100x100_k32       169   10000     2864         2864               8                 169
lattice8_100x100_k200/None 169   10000        0            0               -                 169
half_70x130_k20            240    9100      267          267               3                  57
quarter_130x70_k32         250    9100      104          104               3                  10
odd_53x61_k20              160    3233      455          455               5                 160
row_1x77_k5, column_77x1   63       77       49           49               6                   3
left_half_70x130_k20       220    9100      882          882               6                 220
fine_overflow_64x128_k20   244    8192      993          993               8                 244
super_overflow_96x96_k20   576    9216     1792         1792               8                 576
grid2_30x50_k20            140    1500      329          329               6                 140
outside_48x80_k20          230    3840      567          567               4                 169
lattice32_100x100_k2        16   10000      580          580               4                  16
lattice32_100x100_k4        16   10000      392          392               4                  16
"""

import ctypes

import numpy as np
import pytest

from helpers import idw_exact

pytestmark = pytest.mark.gpu

MAX_ABS, REL_L2 = idw_exact.MAX_ABS, idw_exact.REL_L2


def _values(rng, count):
    """uv ~ N(0, 2) per sample, independent (tied samples differ), rounded to the float32 the kernel is handed."""
    return rng.normal(0.0, 2.0, (count, 2)).astype(np.float32).astype(np.float64)


def _distinct_integers(rng, count, x_lo, x_hi, y_lo, y_hi):
    """``count`` distinct integer positions of [x_lo, x_hi) x [y_lo, y_hi), in shuffled order."""
    w, h = x_hi - x_lo, y_hi - y_lo
    cells = rng.permutation(w * h)[:count]
    return np.column_stack([x_lo + cells % w, y_lo + cells // w]).astype(np.float64)


def _lattice(rng, n, m, step):
    gx, gy = np.meshgrid(np.arange(0, n, step), np.arange(0, m, step))
    xy = np.column_stack([gx.ravel(), gy.ravel()]).astype(np.float64)
    return xy[rng.permutation(len(xy))]


def _fractional(rng, count, n, m, denom):
    """distinct positions on multiples of 1 / denom (what declustering's medians produce), shuffled."""
    xy = np.column_stack([rng.integers(0, n * denom, 4 * count), rng.integers(0, m * denom, 4 * count)])
    xy = np.unique(xy, axis=0)
    return xy[rng.permutation(len(xy))[:count]].astype(np.float64) / denom


def _line_pairs(rng, length, along_x):
    """One-pixel-wide image: samples in pairs mirrored at the pixel line (always equidistant from every pixel of
    it), at distinct positions along the line, offsets 1..5 across it - and three samples on the line itself."""
    pos = rng.permutation(np.arange(-5, length + 5))[:30]
    off = rng.integers(1, 6, pos.size)
    on_line = rng.permutation(np.setdiff1d(np.arange(length), pos))[:3]
    a = np.concatenate([pos, pos, on_line]).astype(np.float64)
    b = np.concatenate([off, -off, np.zeros(3)]).astype(np.float64)
    xy = np.column_stack([a, b] if along_x else [b, a])
    return xy[rng.permutation(len(xy))]


def _case(name):
    """-> dict(xy, uv, xgrid, ygrid, kw, floor).  Shapes are (m, n) = (rows, columns)."""
    kw = {"k": 20}
    floor = 100
    xgrid = ygrid = None
    if name in ("int200_48x80_k20",):
        # L = 200 <= kSuperCap: the supertile lists fit; at 5 pixels between samples a tile's ring (four half
        # diagonals of 8.3 pixels thick) holds far more than 8 -> the replace-the-maximum set add_nearest<20>; the
        # tiles in the middle see more than kFineCap samples -> brute force beside them
        rng = np.random.default_rng(101)
        m, n = 48, 80
        xy = _distinct_integers(rng, 200, 0, n, 0, m)
    elif name in ("int150_64x64_k5", "int150_64x64_k1", "int150_64x64_k5_power2"):
        # one supertile exactly; small k, thick ring: no certain samples, add_nearest<8> picks all k (KMAX 8);
        # k = 1: equidistant NEAREST samples, r = 1 of |T| = 2; power 2 / offset 0.1: the powf weight
        rng = np.random.default_rng(202)
        m, n = 64, 64
        xy = _distinct_integers(rng, 150, 0, n, 0, m)
        kw = {"k": 1} if name.endswith("k1") else {"k": 5}
        if name.endswith("power2"):
            kw.update(power=2.0, dist_offset=0.1)
    elif name.startswith("lattice8_100x100_k"):
        # 13 x 13 samples, spacing 8: tie groups of 4 and 8 by symmetry; k on both sides of each KMAX instantiation
        # (8 / 20 / 32): add_nearest<8> at k = 8, add_nearest<KMAX> with KMAX 20 / 32 above, a few tiles at the
        # image corners with rings of <= 8; k = None and k = 200 >= L = 169: the all-samples path, no selection
        rng = np.random.default_rng(303)
        m, n = 100, 100
        xy = _lattice(rng, n, m, 8)
        kk = name.split("_k")[1]
        kw = {"k": None if kk == "None" else int(kk)}
        if kw["k"] is None or kw["k"] >= len(xy):
            floor = 0
    elif name == "half_70x130_k20":
        # half-integer positions (medians of two integers), image wider than a supertile: three supertiles per row band;
        # L <= kSuperCap (a supertile's reach covers these small images, so a longer list would be brute force everywhere)
        rng = np.random.default_rng(404)
        m, n = 70, 130
        xy = _fractional(rng, 240, n, m, 2)
    elif name == "quarter_130x70_k32":
        # quarter-integer positions, KMAX 32, two supertile rows + a 2-row remainder
        rng = np.random.default_rng(514)  # (ties are rare on quarter integers: a seed with >= 100 of them)
        m, n = 130, 70
        xy = _fractional(rng, 250, n, m, 4)
        kw = {"k": 32}
    elif name == "odd_53x61_k20":
        # neither a multiple of the fine tile (16 x 8) nor of the supertile: partial tiles on both edges
        rng = np.random.default_rng(606)
        m, n = 53, 61
        xy = _distinct_integers(rng, 160, 0, n, 0, m)
    elif name in ("row_1x77_k5", "column_77x1_k5"):
        # one-pixel-wide images: fine tiles with one live row / one live column of lanes
        rng = np.random.default_rng(707)
        along_x = name.startswith("row")
        m, n = (1, 77) if along_x else (77, 1)
        xy = _line_pairs(rng, 77, along_x)
        kw = {"k": 5}
        floor = 40
    elif name == "left_half_70x130_k20":
        # samples only in the left half: the right supertile is far from all of them - a wide bracket, a long list,
        # and every sample of its tiles "certain" or in one thick ring
        rng = np.random.default_rng(808)
        m, n = 70, 130
        xy = _distinct_integers(rng, 220, 0, 65, 0, m)
    elif name == "fine_overflow_64x128_k20":
        # a full 12 x 12 integer block (144 samples) + 100 scattered: L = 244 <= kSuperCap, so both supertile lists fit,
        # but the tiles of the left supertile see more than kFineCap = 96 samples within their reach -> brute force
        # (TopK) per tile, beside tiles of the right supertile on the ordinary path; the one-level kernel
        # (kCandCap = 512 > L) never overflows here
        rng = np.random.default_rng(909)
        m, n = 64, 128
        gx, gy = np.meshgrid(np.arange(26, 38), np.arange(26, 38))
        block = np.column_stack([gx.ravel(), gy.ravel()])
        rest = _distinct_integers(rng, 400, 0, n, 0, m)
        rest = rest[~((rest[:, 0] >= 26) & (rest[:, 0] < 38) & (rest[:, 1] >= 26) & (rest[:, 1] < 38))][:100]
        xy = np.concatenate([block, rest]).astype(np.float64)
        xy = xy[rng.permutation(len(xy))]
    elif name.startswith("lattice32_100x100_k"):
        # 4 x 4 samples, spacing 32 (the benchmark's density, ~130 px, scaled to a small image): few samples near a
        # tile's bracket -> rings of <= 8 samples, ranked pairwise (idw_small_ring2); ties along the bisectors
        rng = np.random.default_rng(1313)
        m, n = 100, 100
        xy = _lattice(rng, n, m, 32)
        kw = {"k": int(name.split("_k")[1])}
    elif name == "super_overflow_96x96_k20":
        # a full 24 x 24 integer block, 576 samples > kSuperCap = 256 (and > kCandCap = 512): every supertile list
        # overflows -> all tiles of the two-level kernels take the brute-force path (tie groups up to 8 at k = 20: the
        # group of 12 at squared distance 25 holds ranks 70 to 81)
        rng = np.random.default_rng(1010)
        m, n = 96, 96
        gx, gy = np.meshgrid(np.arange(36, 60), np.arange(36, 60))
        xy = np.column_stack([gx.ravel(), gy.ravel()]).astype(np.float64)
        xy = xy[rng.permutation(len(xy))]
    elif name == "grid2_30x50_k20":
        # non-unit grid: nodes and samples on even integers, distances divided by the mean spacing 2
        rng = np.random.default_rng(1111)
        xgrid, ygrid = np.arange(0, 100, 2.0), np.arange(0, 60, 2.0)
        m, n = ygrid.size, xgrid.size
        xy = 2.0 * _distinct_integers(rng, 140, 0, 50, 0, 30)
    elif name == "outside_48x80_k20":
        # integer samples up to 5 pixels outside the image on every side
        rng = np.random.default_rng(1212)
        m, n = 48, 80
        xy = _distinct_integers(rng, 230, -5, n + 5, -5, m + 5)
    else:
        raise KeyError(name)
    if xgrid is None:
        xgrid, ygrid = np.arange(n, dtype=np.float64), np.arange(m, dtype=np.float64)
    return {"xy": xy, "uv": _values(rng, len(xy)), "xgrid": xgrid, "ygrid": ygrid, "kw": kw, "floor": floor,
            "integer": bool(np.all(xy == np.round(xy)))}


CASES = [
    "int200_48x80_k20", "int150_64x64_k5", "int150_64x64_k1", "int150_64x64_k5_power2",
    "lattice8_100x100_k8", "lattice8_100x100_k9", "lattice8_100x100_k20", "lattice8_100x100_k21",
    "lattice8_100x100_k32", "lattice8_100x100_k200", "lattice8_100x100_kNone",
    "half_70x130_k20", "quarter_130x70_k32", "odd_53x61_k20", "row_1x77_k5", "column_77x1_k5",
    "left_half_70x130_k20", "fine_overflow_64x128_k20", "super_overflow_96x96_k20", "grid2_30x50_k20",
    "outside_48x80_k20", "lattice32_100x100_k2", "lattice32_100x100_k4",
]

_CACHE = {}


def prepared(name):
    """The case, its oracle (computed once, shared by the three tests of the case, never modified) and the
    CPU-side preconditions: distinct float32 positions, exact squared distances, enough discriminating pixels."""
    if name in _CACHE:
        return _CACHE[name]
    c = _case(name)
    xy, xgrid, ygrid = c["xy"], c["xgrid"], c["ygrid"]
    assert max(ygrid.size, xgrid.size) <= 130
    assert len(np.unique(xy, axis=0)) == len(xy)
    assert idw_exact.squared_distances_exact(xy, xgrid, ygrid)
    ex = idw_exact.IdwExact(xy, c["uv"], xgrid, ygrid, **c["kw"])
    c["exact"] = ex
    c["discriminating"] = ex.discriminating()
    print("%s: L=%d k=%s tie pixels %d of %d (largest tie group %d), discriminating %d, samples on a node %d"
          % (name, len(xy), c["kw"]["k"], ex.n_tie, ex.m * ex.n, ex.largest_group, c["discriminating"], ex.on_node))
    if c["floor"] == 0:
        assert ex.n_tie == 0  # k >= L: every sample is a member
    else:
        assert c["discriminating"] >= c["floor"]
    if c["integer"]:
        assert ex.on_node >= 1  # d = 0: a sample exactly on a node
    _CACHE[name] = c
    return c


def _device_field(c):
    from pysteps_amd.utils.interpolate import idw_to_device

    (x0, dx), (y0, dy) = idw_exact.grid_axis(c["xgrid"]), idw_exact.grid_axis(c["ygrid"])
    out = idw_to_device(c["xy"], c["uv"], c["ygrid"].size, c["xgrid"].size, x0=x0, dx=dx, y0=y0, dy=dy, **c["kw"])
    return out.to_host()


def default_field(name):
    c = prepared(name)
    if "got" not in c:
        got = _device_field(c)
        assert got.dtype == np.float32 and got.shape == (2, c["ygrid"].size, c["xgrid"].size)
        assert np.isfinite(got).all()
        c["got"] = got
    return c["got"]


def _within_bars(got, want):
    from conftest import rel_l2

    err, rel = float(np.max(np.abs(got - want))), rel_l2(got, want)
    print("max abs %.3g (bar %.0e), relative L2 %.3g (bar %.0e)" % (err, MAX_ABS, rel, REL_L2))
    assert err <= MAX_ABS
    assert rel < REL_L2


@pytest.mark.parametrize("name", CASES)
def test_every_pixel_is_a_valid_selection(name):
    """A: no pixel excluded."""
    ex = prepared(name)["exact"]
    got = default_field(name).astype(np.float64)
    bad, text = ex.invalid(got)
    assert bad == 0, "%d pixels match no r-subset of their tie set:\n%s" % (bad, text)
    _within_bars(got, ex.nearest_valid(got))


@pytest.mark.parametrize("name", CASES)
def test_ties_go_to_the_lower_index(name):
    """B: no pixel excluded."""
    ex = prepared(name)["exact"]
    got = default_field(name).astype(np.float64)
    bad, text = ex.off_rule(got)
    assert bad == 0, "%d pixels differ from S + the r lowest-index members of T:\n%s" % (bad, text)
    _within_bars(got, ex.field)


@pytest.mark.parametrize("name", CASES)
def test_paths_agree_on_all_pixels(name):
    """C: both kernel variants, host and resident entry points."""
    from pysteps_amd import _lib
    from pysteps_amd.utils import idwinterp2d

    c = prepared(name)
    ex = c["exact"]
    got = default_field(name)
    lib = _lib.lib()
    _lib.check(lib.psh_set_option(b"idw_variant", 1))
    try:
        old = _device_field(c)
    finally:
        _lib.check(lib.psh_set_option(b"idw_variant", 0))
    diff = np.abs(old.astype(np.float64) - got.astype(np.float64))
    worst = int(diff.max(axis=0).argmax())
    print("variants differ by at most %.3g, at %s" % (diff.max(), ex.describe(worst)))
    assert diff.max() < 1e-5
    host = idwinterp2d(c["xy"], c["uv"], c["xgrid"], c["ygrid"], **c["kw"])
    assert host.dtype == np.float64 and host.size == got.size
    host = host.reshape(got.shape)  # (the reference's convention squeezes a one-pixel-wide grid away)
    assert np.array_equal(host.astype(np.float32), got) and np.array_equal(host, got.astype(np.float64))


# ---- the resident chain: psh_dense_lk_dev -> vectors_finish -> idw_resident (IdwDyn) ----------------------------------
def _finished_samples(lib, xy, uv, scale, m, n):
    """The sample list vectors_finish hands the interpolation (declustered medians, float32) from the pooled,
    outlier-filtered vectors - as tests/test_lk_sparse_gpu.py drives psh_vectors_finish_host."""
    from pysteps_amd import _lib

    xy, uv = np.ascontiguousarray(xy, np.float64), np.ascontiguousarray(uv, np.float64)
    flags = np.zeros(len(xy), np.uint8)
    oxy, ouv = np.empty((len(xy), 2), np.float32), np.empty((len(xy), 2), np.float32)
    count, mode = ctypes.c_int(0), ctypes.c_int(-1)
    const, reach = np.zeros(2, np.float32), np.zeros(1, np.float32)
    _lib.check(lib.psh_vectors_finish_host(xy.ctypes.data, uv.ctypes.data, flags.ctypes.data, len(xy), float(scale), m,
                                           n, oxy.ctypes.data, ouv.ctypes.data, ctypes.byref(count), ctypes.byref(mode),
                                           const.ctypes.data, reach.ctypes.data), "psh_vectors_finish_host")
    return oxy[: count.value].astype(np.float64), ouv[: count.value].astype(np.float64), mode.value


def test_resident_chain_is_valid_at_ties():
    """One 256 x 256 frame pair, default LK keywords: the dense field of the one-call chain against the oracle on
    the sample list the chain interpolated (163 declustered samples from 291 pooled vectors, 398 tie pixels of
    65536, 72 of them discriminating).  With a dense output the call returns no samples, and without one it
    returns the pooled vectors BEFORE vectors_finish (csrc/dense_lk.hip), so the finished list is reproduced with
    psh_vectors_finish_host.  Its order on the device may differ from the reproduced one: A only.
    Corners sit on integers, the declustered medians on half integers."""
    from pysteps_amd import _lib
    from pysteps_amd.motion.lucaskanade import dense_lucaskanade
    from tools import synth

    m = n = 256
    base = synth.rain_field_db(m, n, seed=11)
    frames = np.stack([base, np.roll(base, (2, 3), axis=(0, 1))])
    pooled_xy, pooled_uv = dense_lucaskanade(frames, dense=False)
    field = dense_lucaskanade(frames)
    assert field.shape == (2, m, n) and np.isfinite(field).all()
    xy, uv, mode = _finished_samples(_lib.lib(), pooled_xy, pooled_uv, 20.0, m, n)
    assert mode == 0 and len(xy) > 20
    grid = np.arange(m, dtype=np.float64)
    assert idw_exact.squared_distances_exact(xy, grid, grid)
    ex = idw_exact.IdwExact(xy, uv, grid, grid, k=20)
    print("resident chain: %d pooled vectors, %d samples, tie pixels %d of %d (largest tie group %d), discriminating %d"
          % (len(pooled_xy), len(xy), ex.n_tie, m * n, ex.largest_group, ex.discriminating()))
    assert ex.n_tie >= 100
    bad, text = ex.invalid(field)
    assert bad == 0, "%d pixels match no r-subset of their tie set:\n%s" % (bad, text)
    _within_bars(field, ex.nearest_valid(field))
