"""Cases of the Lucas-Kanade stage tests (tests/test_lk_stages_cpu.py, tests/test_lk_stages_gpu.py): uint8 frames
built on the host, the census of the routes lk_pyrdown takes for a shape, the point sets of the one-step tracker
test and the sample-to-thread maps of the tracker kernels.  Nothing here touches the device except U8Frame."""

import functools

import numpy as np
from scipy.ndimage import gaussian_filter

SHIFT = (0.4, -0.3)  # (x, y) displacement of the second frame of a tracker case


# ---- frames ----------------------------------------------------------------------------------------------------
def _texture(m, n, seed=0, sigma=3.0):
    """The smooth texture of tests/test_lk_gpu.py."""
    rng = np.random.default_rng(seed)
    g = gaussian_filter(rng.standard_normal((m, n)), sigma, mode="wrap")
    return ((g - g.min()) / (g.max() - g.min()) * 40.0 - 15.0).astype(np.float32)


def smooth(m, n, seed):
    from oracle import lk_opencv as olk

    a = _texture(m, n, seed)
    return olk.to_uint8(a, np.ones((m, n), bool), a.min(), a.max(), a.min())


def binary(m, n, seed):
    """i.i.d. 0 / 255: every neighbourhood holds both extremes."""
    return (np.random.default_rng(seed).integers(0, 2, (m, n)) * 255).astype(np.uint8)


def edges(m, n, seed, longest=12, board=2):
    """0 / 255 steps along both axes (runs of 2 .. ``longest`` pixels) with a block of one-pixel checkerboard over
    1 / ``board`` of each axis."""
    rng = np.random.default_rng(seed)

    def runs(length):
        out = np.zeros(length, np.int64)
        at, v = 0, int(rng.integers(0, 2))
        while at < length:
            k = int(rng.integers(2, longest + 1))
            out[at:at + k] = v
            at, v = at + k, 1 - v
        return out

    img = runs(n)[None, :] ^ runs(m)[:, None]
    y0, x0 = int(rng.integers(0, max(m // 2, 1))), int(rng.integers(0, max(n // 2, 1)))
    yy, xx = np.mgrid[0:m, 0:n]
    board = (yy >= y0) & (yy < y0 + (m + 1) // board) & (xx >= x0) & (xx < x0 + (n + 1) // board)
    img[board] = ((yy + xx) & 1)[board]
    return (img * 255).astype(np.uint8)


def planes(m, n, seed=0):
    """Constant 0 / 255 half-planes meeting at 45 degrees: 255 between the vertical line x = 60 and the diagonal
    x + y = 170, 0 elsewhere.  Along the vertical line |Ix| is 16 * 255 in every row, which is what fills a
    thread's share of the window sums; the diagonal keeps the gradient matrix regular."""
    yy, xx = np.mgrid[0:m, 0:n]
    return (((xx >= 60) & (xx + yy < 170)) * 255).astype(np.uint8)


FAMILIES = {"smooth": smooth, "binary": binary, "edges": edges, "planes": planes}


def shifted(u8, dx, dy):
    """The frame displaced by (dx, dy) pixels: bilinear resampling at (x - dx, y - dy), borders clamped, rounded."""
    m, n = u8.shape
    ys = np.clip(np.arange(m) - dy, 0, m - 1)
    xs = np.clip(np.arange(n) - dx, 0, n - 1)
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    y1, x1 = np.minimum(y0 + 1, m - 1), np.minimum(x0 + 1, n - 1)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    f = u8.astype(np.float64)
    v = (f[np.ix_(y0, x0)] * (1 - fx) + f[np.ix_(y0, x1)] * fx) * (1 - fy) + \
        (f[np.ix_(y1, x0)] * (1 - fx) + f[np.ix_(y1, x1)] * fx) * fy
    return np.rint(v).astype(np.uint8)


class U8Frame:
    """Stand-in for PreparedFrame that carries the tracker rendering only.  ``lead`` spare bytes in front of the
    frame move its first pixel off the allocation's alignment."""

    def __init__(self, u8, lead=0):
        from pysteps_amd.device import DeviceArray

        u8 = np.ascontiguousarray(u8, dtype=np.uint8)
        self.shape = u8.shape
        buf = DeviceArray.from_host(np.concatenate([np.zeros(lead, np.uint8), u8.ravel()]))
        self.track_u8 = DeviceArray(u8.shape, np.uint8, ptr=buf.ptr + lead, owner=buf)
        self.ptr = self.track_u8.ptr


# ---- (a) pyramid cases and the routes of lk_pyrdown ------------------------------------------------------------
# (rows, cols, window, max_level)
PYR_CASES = [
    (256, 256, (21, 21), 3),   # rows aligned: fast interior lanes, reflected border lanes
    (130, 131, (9, 7), 3),     # n % 4 != 0 at level 0
    (257, 255, (9, 7), 3),
    (100, 260, (9, 7), 3),     # 260 -> 130 -> 65: the alignment changes from level to level
    (96, 264, (9, 7), 3),      # 264 -> 132 -> 66; on = 132 aligned
    (96, 268, (9, 7), 3),      # on = 134 not aligned, source aligned
    (96, 104, (9, 7), 3),
    (40, 23, (5, 5), 3),       # a level narrower than 16 columns
    (33, 61, (5, 5), 3),       # ... and one of exactly 16
    (66, 96, (9, 7), 3),       # om = 33: the second half of the row walk is skipped
    (90, 96, (9, 7), 3),       # om = 45: ... is cut short
    (48, 1100, (5, 5), 3),     # several workgroups in x
    (301, 203, (9, 7), 3),     # odd at every level
]
PYR_SMOOTH = [(256, 256, (21, 21), 3), (301, 203, (9, 7), 3)]
PYR_UNALIGNED = (64, 128, (9, 7), 3)  # rows of a multiple of 4 bytes behind an odd number of spare bytes
ROUTES = ("fast", "border_bytes", "unaligned_bytes", "small_reflect", "store_dword", "store_bytes", "rows_full",
          "half1_cut", "half2_skipped", "half2_cut", "blocks_x", "blocks_y")


def level_shapes(m, n, win, max_level):
    """buildOpticalFlowPyramid: a level is kept while it is larger than the window."""
    out = [(m, n)]
    for _ in range(max_level):
        r, q = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        if q <= win[0] or r <= win[1]:
            break
        out.append((r, q))
    return out


def pyrdown_routes(m, n, om, on, src_aligned=True):
    """The routes one lk_pyrdown launch takes, from the kernel's predicates: a lane owns output columns
    ox .. ox + 3 (ox a multiple of 4, ox < on), a wave 8 output rows in two halves of 4."""
    routes = set()
    rows_aligned = n % 4 == 0 and src_aligned
    for ox in range(0, on, 4):
        fast = rows_aligned and 2 * ox - 4 >= 0 and 2 * ox + 12 <= n
        if fast:
            routes.add("fast")
        elif n < 16:
            routes.add("small_reflect")
        else:
            routes.add("border_bytes" if rows_aligned else "unaligned_bytes")
    routes.add("store_dword" if on % 4 == 0 else "store_bytes")
    if om >= 8:
        routes.add("rows_full")
    if om % 8:
        if om % 8 < 4:
            routes.add("half1_cut")
        if om % 8 <= 4:
            routes.add("half2_skipped")
        else:
            routes.add("half2_cut")
    if on > 256:
        routes.add("blocks_x")
    if om > 32:
        routes.add("blocks_y")
    return routes


def case_routes(m, n, win, max_level, lead=0):
    shapes = level_shapes(m, n, win, max_level)
    routes = set()
    for l in range(1, len(shapes)):
        # levels above 0 live in a block aligned to 256 bytes; level 0 is the caller's pointer
        routes |= pyrdown_routes(*shapes[l - 1], *shapes[l], src_aligned=(l > 1 or lead % 4 == 0))
    return routes


# ---- (b) gradient image ----------------------------------------------------------------------------------------
SCHARR_WINDOWS = [(62, 20), (64, 64)]
SCHARR_SHAPES = [(130, 131), (200, 256), (67, 193)]  # partial 64 x 4 tiles in both directions

# ---- (c) one tracker step --------------------------------------------------------------------------------------
TRACK_SHAPE = (128, 160)
ROWS_MAX_WIN = 61  # kRowsMaxWin
# window -> instantiation, restated from launch_lk_track
STEP_WINDOWS = [(5, 5), (9, 7), (21, 21), (50, 50), (61, 33), (15, 61), (62, 20), (63, 40), (64, 64), (64, 3)]


def instantiation(win):
    w, h = win
    if w <= ROWS_MAX_WIN:
        rows = (h + 3) // 4
        return "rows", 8 if rows <= 8 else 13 if rows <= 13 else 16
    per = (w * h + 255) // 256
    return "gather", 4 if per <= 4 else 10 if per <= 10 else 16


def case_id(win, family):
    kind, k = instantiation(win)
    return "%dx%d-%s%d-%s" % (win[0], win[1], kind, k, family)


STEP_CASES = [(win, fam) for win in STEP_WINDOWS for fam in ("smooth", "binary", "edges")]
# the constructed frame that fills the sums, on the two instantiations with 16 samples per thread
STEP_CASES += [((64, 64), "planes"), ((15, 61), "planes")]
ILL_CONDITIONED = 1e-3  # px: a bound above this is a nearly singular matrix
MIN_MARGIN = 4.0        # status decisions at least this many noise widths from their thresholds


# seeds are settled on the oracle alone (tests/test_lk_stages_cpu.py: enough points take a step, none sits at a
# threshold); 5 x 5 windows on steps two or three pixels apart are flat more often than the others
STEP_SEEDS = {((5, 5), "edges"): 1192}


def flat_block(shape, win):
    """Rows and columns of the constant block at the bottom border that the flat point's window (half of it
    below the image, where it reflects) and its gradient stencil stay inside."""
    m, n = shape
    w, h = win
    x0 = 30
    return slice(m - (h // 2 + 5), m), slice(x0, x0 + w + 6)


def flat_point(shape, win):
    m, _ = shape
    cols = flat_block(shape, win)[1]
    return (cols.start + 3 + (win[0] - 1) * 0.5 + 0.25, m - 1.0)


def step_points(shape, win, seed):
    """About 40 points (x, y) float32 for a window; see the groups below."""
    m, n = shape
    w, h = win
    hx, hy = (w - 1) * 0.5, (h - 1) * 0.5
    rng = np.random.default_rng(seed)
    pts = []
    # interior, fractional positions: the whole window inside the image
    for _ in range(14):
        pts.append((rng.uniform(hx + 2, n - 3 - hx), rng.uniform(hy + 2, m - 3 - hy)))
    # the window crosses one border each (about 40 % and about 20 % of it outside)
    for f in (0.4, 0.2):
        pts += [(hx - f * w + 0.3, m * 0.37), (n - 1 - hx + f * w + 0.6, m * 0.61),
                (n * 0.23, hy - f * h + 0.7), (n * 0.71, m - 1 - hy + f * h + 0.2)]
    # the four corners of the image
    pts += [(0.0, 0.0), (n - 1.0, 0.0), (0.0, m - 1.0), (n - 1.0, m - 1.0)]
    # exactly integer / half-integer coordinates (the weights round there), window inside and across a border
    cx, cy = n // 2, m // 2
    pts += [(cx, cy), (cx + 17, cy - 9), (3.0, cy + 5), (cx + 0.5, cy + 0.5), (cx - 20.5, cy + 11.5),
            (cx + 8.5, 2.5), (cx - 7, cy + 3.5), (cx + 12.5, cy - 14)]
    # the last window positions accepted: floor(p - half) = -w and cols - 1 (-h and rows - 1) ...
    pts += [(hx - w + 0.25, m * 0.45), (hx + n - 1 + 0.5, m * 0.55), (n * 0.4, hy - h + 0.75), (n * 0.6, hy + m - 1 + 0.25)]
    # ... and one pixel beyond: rejected
    pts += [(hx - w - 0.75, m * 0.5), (hx + n + 0.25, m * 0.5), (n * 0.5, hy - h - 0.5), (n * 0.5, hy + m + 0.5)]
    # a flat patch: minimum eigenvalue below the threshold
    pts.append(flat_point(shape, win))
    return np.array(pts, dtype=np.float32)


def planes_points(win):
    """Windows on the vertical line of planes() with the diagonal crossing them, at integer window positions
    (weights 16384, 0, 0, 0) and at fractional ones."""
    w, h = win
    hx, hy = (w - 1) * 0.5, (h - 1) * 0.5
    tops = [(60 - w // 2 + dx, 107 - h + dy) for dx in (-3, 0, 2) for dy in (-4, 0, 1)]
    pts = [(x + hx, y + hy) for x, y in tops]
    pts += [(x + hx + fx, y + hy + fy) for (x, y), fx, fy in zip(tops, np.linspace(0.1, 0.9, 9), np.linspace(0.8, 0.2, 9))]
    pts += [(x + hx + 0.5, y + hy) for x, y in tops[:4]]
    return np.array(pts, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def step_case(win, family):
    """(prev_u8, next_u8, points) of a one-step case."""
    m, n = TRACK_SHAPE
    seed = STEP_SEEDS.get((win, family), 1000 + 37 * win[0] + win[1])
    if family == "edges":
        # steps close enough together that every window holds edges of both directions
        a = edges(m, n, seed, longest=max(2, min(12, min(win) // 2 + 1)), board=4)
    else:
        a = FAMILIES[family](m, n, seed)
    if family == "planes":
        # the next frame two whole pixels to the left: at the line's columns diff is 255 * 32 where |Ix| is 16 * 255
        b = np.concatenate([a[:, 2:], a[:, -2:]], axis=1)
        return a, b, planes_points(win)
    a = a.copy()
    a[flat_block((m, n), win)] = 0 if family != "smooth" else 128
    return a, shifted(a, *SHIFT), step_points((m, n), win, seed)


@functools.lru_cache(maxsize=None)
def step_oracle(win, family):
    """first_step of a case, computed once and shared."""
    from oracle import lk_opencv as olk

    a, b, pts = step_case(win, family)
    return olk.first_step(a, b, pts, win)


def compared(res):
    """Points whose step is held to the bound: the iteration ran, well conditioned, decisions clear of noise."""
    return res["stepped"] & (res["bound"].max(axis=1) <= ILL_CONDITIONED) & (res["margin"] >= MIN_MARGIN)


# ---- (d) full tracking on saturated contrast -------------------------------------------------------------------
FULL_SHAPE = (160, 192)
FULL_CASES = [(win, fam) for win in ((21, 21), (64, 64)) for fam in ("binary", "edges")]


@functools.lru_cache(maxsize=None)
def full_case(win, family):
    m, n = FULL_SHAPE
    seed = 500 + win[0]
    a = FAMILIES[family](m, n, seed)
    pts = step_points((m, n), win, seed)
    pts = np.concatenate([pts[:2], pts[14:42]])  # two interior points and the border, corner, rounding and limit sets
    return a, shifted(a, *SHIFT), pts


# ---- the sample-to-thread maps of the trackers ------------------------------------------------------------------
GRAD_MAX = 16 * 255        # |Ix|, |Iy| of calcSharrDeriv on uint8
DIFF_MAX = 255 * 32        # |J - I| of the patches (5 fraction bits)
SHARE_SAMPLES = 16         # samples per thread at most (lk_track<16>, lk_track_rows<16>)


def thread_shares(values, win):
    """Sums of ``values`` (h, w) over the window samples of each thread of the kernel that takes ``win``:
    lk_track<kPer>: thread t holds samples t, t + 256, ... in row-major order; lk_track_rows<ROWS>: lane = window
    column, wave k the rows k * ROWS ... + ROWS."""
    w, h = win
    kind, k = instantiation(win)
    if kind == "gather":
        flat = values.reshape(-1)
        return np.array([flat[t::256].sum() for t in range(min(256, flat.size))])
    return np.array([values[r0:r0 + k, x].sum() for r0 in range(0, h, k) for x in range(w)])
