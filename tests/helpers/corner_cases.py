"""Cases of the corner-stage tests (tests/test_corner_stages_cpu.py, tests/test_corner_stages_gpu.py): seeded uint8
images that are hard for the Shi-Tomasi front end (lk_corner_response_cols, lk_corner_response_nms, lk_max_final,
lk_corner_select in pysteps_amd/csrc/lk.hip), NaN masks, the shapes that put an image edge on every seam of the
kernels' tilings, the census of candidates per tile and a restatement of the image rows a wave of the response
kernels loads.  Nothing here touches the device."""

import functools

import numpy as np

# ---- geometry of the kernels, restated from lk.hip -------------------------------------------------------------
CRN_ROWS = 32      # kCrnRows: output rows per wave of the response passes
NMS_KEYS = 64      # kNmsKeys: output slots per wave of the fused pass
SEL_COLS = 62      # kSelCols: columns per wave of lk_corner_select
SEL_ROWS = 16      # rows per group of lk_corner_select
BLOCK_SIZES = (1, 3, 5, 7)


def crn_cols(block_size):
    """crn_cols(): output columns per wave of lk_corner_response_cols; the fused pass judges two fewer."""
    return 64 - 2 * (block_size // 2 + 1)


def fused_tile(block_size):
    """(rows, columns) a wave of lk_corner_response_nms judges."""
    return CRN_ROWS, crn_cols(block_size) - 2


# ---- image families --------------------------------------------------------------------------------------------
def noise(m, n, seed):
    """Uniform 0 .. 255: a 3x3 maximum every nine pixels or so, no two responses alike."""
    return np.random.default_rng(seed).integers(0, 256, (m, n)).astype(np.uint8)


def two_level(m, n, seed):
    """Random 0 / 255: the largest gradients everywhere, the border included."""
    return (np.random.default_rng(seed).integers(0, 2, (m, n)) * 255).astype(np.uint8)


def period4(m, n, seed=0):
    """The 4x4 tile of 2x2 blocks, repeated: with block_size >= 3 nearly every response is the same number."""
    tile = np.array([[0, 0, 255, 255]] * 2 + [[255, 255, 0, 0]] * 2, dtype=np.uint8)
    return np.tile(tile, ((m + 3) // 4, (n + 3) // 4))[:m, :n].copy()


def blocks8(m, n, seed):
    """8x8 constant blocks of two levels: flat interiors (zero response) and equal responses along the block edges."""
    coarse = np.random.default_rng(seed).integers(0, 2, ((m + 7) // 8, (n + 7) // 8))
    return np.where(np.kron(coarse, np.ones((8, 8), np.int64))[:m, :n] > 0, 200, 40).astype(np.uint8)


def ramp_impulse(m, n, seed):
    """A horizontal ramp with isolated 255 pixels: one in every corner, one on every edge row and column, a few
    inside.  The strong responses sit where the walk is mirrored."""
    img = np.broadcast_to((np.arange(n) * 200 // max(n - 1, 1)).astype(np.uint8), (m, n)).copy()
    spots = [(0, 0), (0, n - 1), (m - 1, 0), (m - 1, n - 1), (0, n // 2), (m - 1, n // 3), (m // 2, 0), (m // 3, n - 1)]
    rng = np.random.default_rng(seed)
    spots += [(int(rng.integers(0, m)), int(rng.integers(0, n))) for _ in range(4)]
    for y, x in spots:
        img[y, x] = 255
    return img


def rain(m, n, seed):
    """tools/synth.rain_field_db in the oracle's uint8 rendering."""
    from oracle import lk_opencv as olk
    from tools import synth

    if m * n == 1:
        return np.zeros((m, n), np.uint8)  # (one pixel has no spread to scale by)
    db = synth.rain_field_db(m, n, seed=seed, sigma=max(m / 64.0, 2.0))
    return olk.to_uint8(db, np.ones((m, n), bool), db.min(), db.max(), db.min())


def flat(m, n, seed=0):
    return np.full((m, n), 77, np.uint8)


FAMILIES = {"noise": noise, "two_level": two_level, "period4": period4, "blocks8": blocks8,
            "ramp_impulse": ramp_impulse, "rain": rain, "flat": flat}


@functools.lru_cache(maxsize=None)
def image(family, m, n):
    """The image of a family at a shape (seeded by the shape); shared, read-only."""
    img = FAMILIES[family](m, n, 1000 * m + n)
    img.setflags(write=False)
    return img


# ---- NaN masks -------------------------------------------------------------------------------------------------
NAN_KINDS = ("none", "corner_block", "pixel", "row")


def nan_mask(kind, m, n):
    """True where the cleaned frame is missing."""
    mask = np.zeros((m, n), bool)
    if kind == "corner_block":
        mask[: max(m // 3, 1), : max(n // 4, 1)] = True
    elif kind == "pixel":
        mask[m // 2, (2 * n) // 3] = True
    elif kind == "row":
        mask[(2 * m) // 3, :] = True
    elif kind != "none":
        raise ValueError(kind)
    return mask


def clean_plane(mask):
    """A float32 plane whose only role is its NaN pattern."""
    plane = np.zeros(mask.shape, np.float32)
    plane[mask] = np.nan
    return plane


# ---- shapes ----------------------------------------------------------------------------------------------------
SHAPES_DEGENERATE = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 70), (7, 9)]
# heights at which the response kernels' preload used to reach a row in front of the image
SHAPES_PRELOAD = [(6, 20), (8, 61), (9, 64), (11, 57), (12, 117), (13, 20), (16, 59)]
SHAPES_COLUMN_SEAMS = [(9, 56), (9, 57), (10, 58), (10, 59), (33, 60), (33, 61), (34, 62), (34, 63), (12, 124), (12, 125)]
SHAPES_ROW_SEAMS = [(31, 70), (32, 70), (33, 70), (128, 66), (129, 117)]
SHAPES_SELECT = [(16, 62), (17, 63), (65, 249), (40, 130), (257, 255)]
SHAPES = SHAPES_DEGENERATE + SHAPES_PRELOAD + SHAPES_COLUMN_SEAMS + SHAPES_ROW_SEAMS + SHAPES_SELECT
HARD_SHAPES = [(40, 130), (129, 117)]


# ---- candidates per tile ---------------------------------------------------------------------------------------
def tile_counts(keys, m, n, tile_rows, tile_cols):
    """Number of candidate keys (low word: y * n + x) in every tile of ``tile_rows`` x ``tile_cols`` pixels, the
    tiling starting at pixel (0, 0)."""
    addr = (np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ty, tx = (addr // n) // tile_rows, (addr % n) // tile_cols
    counts = np.zeros(((m + tile_rows - 1) // tile_rows, (n + tile_cols - 1) // tile_cols), np.int64)
    np.add.at(counts, (ty, tx), 1)
    return counts


# ---- the rows a wave of the response kernels loads -------------------------------------------------------------
def few_rows_bound(block_size, fused):
    """Heights below this take the general (repeated) reflection in the response kernels."""
    r = block_size // 2
    h = r + 1
    return max(2 * h + (4 if fused else 2), 3 * block_size - r + (1 if fused else 0))


def few_rows_bound_before(block_size, fused):
    """The bound before the preload's reach was taken into account (2 H + 2 / 2 H + 4)."""
    return 2 * (block_size // 2 + 1) + (4 if fused else 2)


def _reflect101(i, n):
    if n == 1:
        return 0
    i = abs(i)
    if i >= n:
        period = 2 * (n - 1)
        i %= period
        if i >= n:
            i = period - i
    return i


def rows_loaded(m, block_size, fused, bound=few_rows_bound):
    """Every image row index a wave of lk_corner_response_cols (``fused`` False) or lk_corner_response_nms (True)
    forms for a load on an image of ``m`` rows, restated from the kernels' loop bounds: sequence rows 0, 1 and
    2 .. BS + 1 ahead of the walk, then BS rows ahead of every step of BS product rows; sequence row i is image row
    yb - H + i, reflected once - or as often as needed where the image has few rows."""
    bs = block_size
    h = bs // 2 + 1
    few_rows = m < bound(bs, fused)

    def row_of(y):
        if few_rows:
            return _reflect101(y, m)
        y = abs(y)
        return 2 * m - 2 - y if y >= m else y

    rows = []
    for wave in range((m + CRN_ROWS - 1) // CRN_ROWS):  # the waves whose first (judged) row lies in the image
        if fused:
            yb = wave * CRN_ROWS - 1
            last_p = min(CRN_ROWS + 2, m - yb) + bs - 1
        else:
            yb = wave * CRN_ROWS
            last_p = min(CRN_ROWS, m - yb) + bs - 1
        seq = list(range(0, bs + 2))
        for base in range(1, last_p + 1, bs):
            seq += [base + bs + 1 + j for j in range(bs)]
        rows += [row_of(yb - h + i) for i in seq]
    return rows


def heights_out_of_range(block_size, fused, bound=few_rows_bound, heights=range(1, 201)):
    """Heights at which some load leaves [0, m)."""
    return [m for m in heights if any(not 0 <= y < m for y in rows_loaded(m, block_size, fused, bound))]
