"""Linear and salient blending (pysteps/blending/linear_blending.py) for the tests: the case list, a seeded field
generator and an independent NumPy restatement of the blend stage.

The restatement follows the reference's ``forecast`` from the member pairing on, with NumPy's own arithmetic (so dtype
promotion and the rounding of the Python-float weights are NumPy's), but never repeats a member - it reads through the
index maps - and takes the dense ranks from ``np.unique(..., return_inverse=True)`` instead of ``scipy.stats.rankdata``.
tests/test_blending_cpu.py holds it to the goldens of the unmodified reference bit for bit.

Fields: rain cells quantised to 1/8 mm/h over a dry background, NaN borders of a width that changes with the lead time
in the nowcast.  Every case is rebuilt from its recipe; the golden file stores the SHA-256 of the inputs it was made from.
"""

import hashlib

import numpy as np

# (timesteps, timestep, start_blending, end_blending): weights 0, 1/3, 2/3, 1, 1 - before, inside and after the window
SCHEDULE = dict(timesteps=5, timestep=5, start_blending=5, end_blending=20)
SHORT = dict(timesteps=3, timestep=5, start_blending=5, end_blending=15)  # weights 0, 1/2, 1

# name -> recipe; kn / kw: members (0: a 3-d stack), special: what the generator does on top
CASES = {
    "single_37x53": dict(kn=0, kw=0, m=37, n=53, seed=1),
    "plain_64x96": dict(kn=0, kw=0, m=64, n=96, seed=2),
    "ens3_40x50": dict(kn=3, kw=3, m=40, n=50, seed=3),
    "big_300x300": dict(kn=0, kw=0, m=300, n=300, seed=4, schedule="short", dtypes=("float32", "float32")),
    "nowcast_zero": dict(kn=0, kw=0, m=37, n=53, seed=5, special="nowcast_zero"),
    "nwp_zero": dict(kn=0, kw=0, m=37, n=53, seed=6, special="nwp_zero"),
    "equal_fields": dict(kn=0, kw=0, m=37, n=53, seed=7, special="equal"),
    "all_distinct": dict(kn=0, kw=0, m=37, n=53, seed=8, special="distinct"),
    "last_bit": dict(kn=0, kw=0, m=37, n=53, seed=9, special="last_bit"),
    "negative_zero": dict(kn=0, kw=0, m=37, n=53, seed=10, special="negative_zero"),
    "dry_95": dict(kn=0, kw=0, m=64, n=96, seed=11, special="dry"),
    "nwp_inf": dict(kn=0, kw=0, m=37, n=53, seed=12, special="nwp_inf"),
    "no_fill": dict(kn=0, kw=0, m=37, n=53, seed=13, fill_nwp=False),
    "f32_f32": dict(kn=0, kw=0, m=37, n=53, seed=14, dtypes=("float32", "float32")),
    "f32_f64": dict(kn=0, kw=0, m=37, n=53, seed=15, dtypes=("float32", "float64")),
    "f64_f32": dict(kn=0, kw=0, m=37, n=53, seed=16, dtypes=("float64", "float32")),
    "f32_f32_ens": dict(kn=2, kw=2, m=40, n=50, seed=17, dtypes=("float32", "float32")),
    "pair_1_3": dict(kn=1, kw=3, m=24, n=31, seed=18),
    "pair_3_1": dict(kn=3, kw=0, m=24, n=31, seed=19),
    "pair_5_2": dict(kn=5, kw=2, m=24, n=31, seed=20),
    "pair_2_5": dict(kn=2, kw=5, m=24, n=31, seed=21),
}
PAIRINGS = [(1, 3), (3, 1), (4, 4), (5, 2), (2, 5)]


def schedule(name):
    return dict(SHORT if CASES[name].get("schedule") == "short" else SCHEDULE)


def rain(rng, shape, wet=0.35):
    """A (..., m, n) stack of rain cells in 1/8 steps over a dry background."""
    m, n = shape[-2:]
    planes = int(np.prod(shape[:-2], dtype=np.int64))
    yy, xx = np.mgrid[0:m, 0:n]
    out = np.zeros((planes, m, n))
    for p in range(planes):
        for _ in range(max(2, int(wet * 12))):
            cy, cx = rng.uniform(0, m), rng.uniform(0, n)
            s = rng.uniform(0.04, 0.12) * max(m, n) * np.sqrt(wet / 0.35)
            out[p] += rng.uniform(2.0, 30.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    out = np.round(out * 8.0) / 8.0
    out[out < 0.25] = 0.0
    return out.reshape(shape)


def make_case(name):
    """``(precip_nowcast, precip_nwp, kwargs)`` of a case: rain-rate stacks and the arguments of ``blend``."""
    c = CASES[name]
    sch = schedule(name)
    rng = np.random.default_rng(1000 + c["seed"])
    m, n = c["m"], c["n"]
    t_nowcast = int(sch["end_blending"] / sch["timestep"])
    t_nwp = sch["timesteps"] + 1  # one more than is read
    special = c.get("special")
    shape_n = ((c["kn"],) if c["kn"] else ()) + (t_nowcast, m, n)
    shape_w = ((c["kw"],) if c["kw"] else ()) + (t_nwp, m, n)
    wet = 0.04 if special == "dry" else 0.35
    nowcast = rain(rng, shape_n, wet)
    nwp = rain(rng, shape_w, wet)
    if special == "nowcast_zero":
        nowcast[:] = 0.0
    elif special == "nwp_zero":
        nwp[:] = 0.0
    elif special == "equal":
        nwp[..., :t_nowcast, :, :] = nowcast
    elif special == "distinct":
        nowcast = rng.uniform(0.0, 40.0, size=shape_n)
        nwp = rng.uniform(0.0, 40.0, size=shape_w)
    elif special == "last_bit":
        nwp[..., :t_nowcast, :, :] = nowcast
        up = rng.random(shape_n) < 0.3
        down = rng.random(shape_n) < 0.3
        nowcast = np.where(up, np.nextafter(nowcast, np.inf), nowcast)
        nowcast = np.where(down & ~up & (nowcast > 0), np.nextafter(nowcast, -np.inf), nowcast)
    elif special == "negative_zero":
        nowcast[(nowcast == 0) & (rng.random(shape_n) < 0.3)] = -0.0
        nwp[(nwp == 0) & (rng.random(shape_w) < 0.3)] = -0.0
    elif special == "nwp_inf":
        nwp[rng.random(shape_w) < 0.01] = np.inf
        nwp[rng.random(shape_w) < 0.01] = -np.inf
        nwp[rng.random(shape_w) < 0.02] = np.nan
    if special not in ("nowcast_zero", "equal", "distinct", "last_bit"):
        for i in range(t_nowcast):  # NaN borders that grow with the lead time, as an extrapolation leaves them
            b = 1 + i
            nowcast[..., i, :b, :] = np.nan
            nowcast[..., i, :, -(b + 1):] = np.nan
        if special == "nwp_inf":
            nwp[..., 0, 0, 0] = np.inf  # under a nowcast NaN: the fill takes the largest finite value
    dt_n, dt_w = c.get("dtypes", ("float64", "float64"))
    nowcast, nwp = nowcast.astype(dt_n), nwp.astype(dt_w)
    kwargs = dict(sch, fill_nwp=c.get("fill_nwp", True))
    return nowcast, nwp, kwargs


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def weights(timesteps, timestep, start_blending, end_blending):
    """The reference's ``weight_nwp`` per lead time after its clamps."""
    out = []
    for i in range(timesteps):
        t = (i + 1) * timestep
        w = (t - start_blending) / (end_blending - start_blending)
        out.append(0.0 if w <= 0.0 else (1.0 if w >= 1.0 else w))
    return out


def repeat_maps(kn, kw):
    """Index maps equal to what the reference's ``np.repeat`` calls produce, built from them."""
    a, b = np.arange(kn), np.arange(kw)
    k_max, k_min = max(kn, kw), min(kn, kw)
    if k_min != k_max:
        if kw == 1:
            b = np.repeat(b, k_max)
        elif kn == 1:
            a = np.repeat(a, k_max)
        else:
            repeats = [(k_max + i) // k_min for i in range(k_min)]
            if kw == k_min:
                b = np.repeat(b, repeats)
            else:
                a = np.repeat(a, repeats)
    return a, b


def dense_ranks(diff):
    """Dense ranks from 1 and their number, by ``np.unique`` (-0.0 and 0.0 compare equal there as well)."""
    values, inverse = np.unique(diff.ravel(), return_inverse=True)
    return (inverse.reshape(diff.shape) + 1).astype(np.float64), len(values)


def ranked_salience(nowcast, nwp):
    max_n, max_w = np.max(nowcast), np.max(nwp)
    norm_n = np.zeros_like(nowcast) if max_n == 0 else nowcast / max_n
    norm_w = np.zeros_like(nwp) if max_w == 0 else nwp / max_w
    ranks, distinct = dense_ranks(norm_n - norm_w)
    return ranks / float(distinct)


def salience_weight(weight, rs):
    first = (weight * rs) / (weight * rs + (1 - weight) * (1 - rs))
    s1 = np.sqrt(rs * rs + weight**2)
    s2 = np.sqrt((1 - rs) * (1 - rs) + (1 - weight) ** 2)
    return 0.5 * (first + s1 / (s1 + s2))


def blend(precip_nowcast, precip_nwp, timesteps, timestep, start_blending, end_blending, fill_nwp=True, saliency=False):
    """The blend stage restated; inputs are left alone."""
    nowcast = precip_nowcast if precip_nowcast.ndim == 4 else precip_nowcast[None]
    nwp = precip_nwp if precip_nwp.ndim == 4 else precip_nwp[None]
    nwp = nwp[:, 0:timesteps]
    t_nowcast = int(end_blending / timestep)
    if nwp[:, 0:t_nowcast].shape[1] != nowcast.shape[1]:
        raise IndexError("the NWP stack is shorter than the nowcast")
    map_n, map_w = repeat_maps(nowcast.shape[0], nwp.shape[0])
    K = len(map_n)
    out = np.zeros((K,) + nwp.shape[1:], dtype=nwp.dtype)
    with np.errstate(all="ignore"):
        for i, w_nwp in enumerate(weights(timesteps, timestep, start_blending, end_blending)):
            b = np.nan_to_num(nwp[map_w, i], nan=0.0)
            if w_nwp == 1.0:
                out[:, i] = b
                continue
            a = nowcast[map_n, i].copy()
            mask = np.isnan(a)
            a[mask] = b[mask] if fill_nwp else 0.0
            if w_nwp == 0.0:
                out[:, i] = a
            elif saliency:
                ws = salience_weight(1.0 - w_nwp, ranked_salience(a, b))
                out[:, i] = ws * a + (1 - ws) * b
            else:
                out[:, i] = w_nwp * b + (1.0 - w_nwp) * a
    return out[0] if K == 1 else out


# ---- the dB inverse ----------------------------------------------------------------------------------------------
DB_META = {"transform": "dB", "unit": "mm/h", "threshold": -10.0, "zerovalue": -15.0}


def db_field(seed=31, shape=(2, 48, 64)):
    """A float64 field on a 0.25 dB grid: wet pixels from -10 dB (the threshold itself) upwards, dry ones at -15 dB, a
    NaN border."""
    rng = np.random.default_rng(seed)
    r = rain(rng, shape)
    with np.errstate(divide="ignore"):
        db = np.where(r > 0, np.round(10.0 * np.log10(np.maximum(r, 1e-3)) * 4.0) / 4.0, -15.0)
    db[rng.random(shape) < 0.02] = -10.0
    db[rng.random(shape) < 0.02] = -10.25
    db[..., :2, :] = np.nan
    return db


def db_inverse_longdouble(db, threshold_db=-10.0, zerovalue=0.0):
    """``10 ** (db / 10)`` with the quotient rounded to float64 as the reference rounds it and the power in long double;
    the cut in dB, which is the reference's cut in linear units for a monotone power."""
    q = (db / 10.0).astype(np.longdouble)
    with np.errstate(invalid="ignore"):
        out = np.power(np.longdouble(10.0), q)
        out[db < threshold_db] = zerovalue
    return out
