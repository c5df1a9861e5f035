"""The Proesmans motion estimate (pysteps/motion/proesmans.py, _proesmans.pyx) restated stage by stage in float64 NumPy:
the same IEEE operations in the same order as the reference's C (x86-64 gcc -O2 does not contract to FMA), so the
restatement equals the compiled reference bit for bit (tests/test_proesmans_cpu.py, tools/make_golden_proesmans.py).

The reference sweeps each field in place in raster order, a Gauss-Seidel sweep: pixel (y, x) reads its three upper
neighbours and its left neighbour after the sweep wrote them, the other four before.  In t = x + 2 y every pixel
depends only on results of smaller t, so :func:`sweep` evaluates one t at a time, all its pixels and both directions
as one array expression.  :func:`sweep_jacobi` reads everything from the old field: another algorithm, kept for the
test that shows the goldens tell the two apart.

``c_sum``: "sequential" is the reference's raster-order running sum behind K = 0.9 c_sum / c_count; "exact" is
``math.fsum`` (what the device computes, to one rounding)."""

import math

import numpy as np

INTENSITY_SCALE = 1.0 / 255.0


def scale_frames(frames):
    """proesmans.py: the last two frames scaled to [0, 255] over both (left alone when constant)."""
    im = np.stack([frames[-2], frames[-1]]).astype(np.float64)
    im_min, im_max = np.min(im), np.max(im)
    if im_max - im_min > 1e-8:
        im = (im - im_min) / (im_max - im_min) * 255.0
    return im


def pyramid_level(src):
    dh, dw = int(src.shape[0] / 2), int(src.shape[1] / 2)
    return (src[0:2 * dh:2, 0:2 * dw:2] + src[0:2 * dh:2, 1:2 * dw:2] + src[1:2 * dh:2, 0:2 * dw:2]
            + src[1:2 * dh:2, 1:2 * dw:2]) / 4.0


def pyramid(frame, n_levels):
    out = [np.ascontiguousarray(frame, dtype=np.float64)]
    for _ in range(1, n_levels):
        out.append(pyramid_level(out[-1]))
    return out


def gradient_kernels():
    """Kx, Ky as _compute_gradients forms them."""
    s = INTENSITY_SCALE
    Kx = np.array([[1.0 / 8.0 * s, 0.0, -1.0 / 8.0 * s],
                   [2.0 / 8.0 * s, 0.0, -2.0 / 8.0 * s],
                   [1.0 / 8.0 * s, 0.0, -1.0 / 8.0 * s]])
    Ky = np.array([[1.0 / 8.0 * s, 2.0 / 8.0 * s, 1.0 / 8.0 * s],
                   [0.0, 0.0, 0.0],
                   [-1.0 / 8.0 * s, -2.0 / 8.0 * s, -1.0 / 8.0 * s]])
    return Kx, Ky


def gradients(I):
    """The two ``scipy.ndimage.convolve(I, K, mode="constant", cval=0.0)``: the kernel flipped, a running sum that
    starts at 0.0 and takes the non-zero taps in raster order of the flipped kernel, zeros outside the image."""
    m, n = I.shape
    P = np.zeros((m + 2, n + 2))
    P[1:-1, 1:-1] = I
    out = np.empty((2, m, n))
    for k, K in enumerate(gradient_kernels()):
        acc = np.zeros((m, n))
        for a in range(3):
            for b in range(3):
                w = K[2 - a, 2 - b]
                if w != 0.0:
                    acc = acc + w * P[a:a + m, b:b + n]
        out[k] = acc
    return out


def interpolate(I, x, y, lead=None):
    """_linear_interpolate at arrays x, y; I is (h, w), or (k, h, w) with ``lead`` selecting the plane per sample."""
    h, w = I.shape[-2:]
    x0 = np.trunc(x).astype(np.int64)
    y0 = np.trunc(y).astype(np.int64)
    x1 = np.clip(x0 + 1, 0, w - 1)
    y1 = np.clip(y0 + 1, 0, h - 1)
    x0 = np.clip(x0, 0, w - 1)
    y0 = np.clip(y0, 0, h - 1)
    if lead is None:
        Ia, Ib, Ic, Id = I[y0, x0], I[y1, x0], I[y0, x1], I[y1, x1]
    else:
        Ia, Ib, Ic, Id = I[lead, y0, x0], I[lead, y1, x0], I[lead, y0, x1], I[lead, y1, x1]
    wa = (x1 - x) * (y1 - y)
    wb = (x1 - x) * (y - y0)
    wc = (x - x0) * (y1 - y)
    wd = (x - x0) * (y - y0)
    return wa * Ia + wb * Ib + wc * Ic + wd * Id


def consistency_raw(V):
    """The raw c planes of _compute_consistency_maps, -1 where the displaced pixel leaves the image: (2, m, n)."""
    m, n = V.shape[2:]
    yy, xx = np.mgrid[0:m, 0:n]
    c = np.empty((2, m, n))
    for i in range(2):
        xd = xx + V[i, 0]
        yd = yy + V[i, 1]
        inside = (xd >= 0) & (yd >= 0) & (xd < n) & (yd < m)
        xs, ys = np.where(inside, xd, 0.0), np.where(inside, yd, 0.0)
        u = V[i, 0] + interpolate(V[1 - i, 0], xs, ys)
        v = V[i, 1] + interpolate(V[1 - i, 1], xs, ys)
        c[i] = np.where(inside, np.sqrt(u * u + v * v), -1.0)
    return c


def consistency_sum(c_plane, c_sum="sequential"):
    """(c_sum, c_count) of one raw plane."""
    vals = c_plane[c_plane >= 0.0]  # raster order
    if vals.size == 0:
        return 0.0, 0
    if c_sum == "exact":
        return math.fsum(vals.tolist()), int(vals.size)
    return float(np.add.accumulate(vals)[-1]), int(vals.size)


def consistency_K(total, count):
    return 0.9 * total / count if count > 0 else 0.0


def consistency_normalise(c_plane, K):
    if not K > 1e-8:
        return np.ones_like(c_plane)
    g = np.where(c_plane >= 0.0, c_plane, 0.0)
    return np.where(c_plane >= 0.0, 1.0 / (1.0 + (g / K) * (g / K)), 1.0)


def consistency_maps(V, c_sum="sequential"):
    c = consistency_raw(V)
    return np.stack([consistency_normalise(c[i], consistency_K(*consistency_sum(c[i], c_sum))) for i in range(2)])


_NEIGHBOURS = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))


def _update(Vr, Vw, GAMMA, R, G, lam, ys, xs):
    """The reference's pixel update at (ys, xs) of both directions: neighbours read from Vr, results stored to Vw."""
    m, n = R.shape[1:]
    g = [GAMMA[:, ys + dy, xs + dx] for dy, dx in _NEIGHBOURS]
    sw = (g[0] + g[1] + g[2] + g[3]) / 6.0 + (g[4] + g[5] + g[6] + g[7]) / 12.0
    ok = sw > 1e-8
    swd = np.where(ok, sw, 1.0)
    avg = []
    for k in range(2):
        v = [Vr[:, k, ys + dy, xs + dx] for dy, dx in _NEIGHBOURS]
        s = (g[0] * v[0] + g[1] * v[1] + g[2] * v[2] + g[3] * v[3]) / 6.0 \
            + (g[4] * v[4] + g[5] * v[5] + g[6] * v[6] + g[7] * v[7]) / 12.0
        avg.append(np.where(ok, s / swd, 0.0))
    xd = xs + avg[0]
    yd = ys + avg[1]
    inside = (xd >= 0) & (xd < n - 1) & (yd >= 0) & (yd < m - 1)
    lead = np.array([1, 0]).reshape((2,) + (1,) * np.ndim(ys))  # direction j samples frame 1 - j
    It = (interpolate(R, np.where(inside, xd, 0.0), np.where(inside, yd, 0.0), lead) - R[:, ys, xs]) * INTENSITY_SCALE
    gx, gy = G[:, 0, ys, xs], G[:, 1, ys, xs]
    ic = lam * It / (1.0 + lam * (gx * gx + gy * gy))
    Vw[:, 0, ys, xs] = np.where(inside, avg[0] - gx * ic, avg[0])
    Vw[:, 1, ys, xs] = np.where(inside, avg[1] - gy * ic, avg[1])


def fill_edges(V):
    """_fill_edges on both directions of V (2, 2, m, n), in place."""
    V[..., 0, 1:-1] = V[..., 1, 1:-1]
    V[..., -1, 1:-1] = V[..., -2, 1:-1]
    V[..., 1:-1, 0] = V[..., 1:-1, 1]
    V[..., 1:-1, -1] = V[..., 1:-1, -2]
    V[..., 0, 0] = V[..., 1, 1]
    V[..., 0, -1] = V[..., 1, -2]
    V[..., -1, 0] = V[..., -2, 1]
    V[..., -1, -1] = V[..., -2, -2]


def sweep(V, GAMMA, R, G, lam):
    """One iteration's sweep of both directions in the reference's dependency order, then the edge fill; V in place.
    R (2, m, n) frames, G (2, 2, m, n) their gradients, GAMMA (2, m, n)."""
    m, n = R.shape[1:]
    lam = float(lam)
    for t in range(3, (n - 2) + 2 * (m - 2) + 1):
        ys = np.arange(max(1, (t - (n - 2) + 1) // 2), min(m - 2, (t - 1) // 2) + 1)
        _update(V, V, GAMMA, R, G, lam, ys, t - 2 * ys)
    fill_edges(V)


def sweep_jacobi(V, GAMMA, R, G, lam):
    """Every pixel from the old field: NOT the reference's algorithm."""
    m, n = R.shape[1:]
    ys, xs = np.mgrid[1:m - 1, 1:n - 1]
    _update(V.copy(), V, GAMMA, R, G, float(lam), ys, xs)
    fill_edges(V)


def next_level(V_prev, m_next, n_next):
    """_initialize_next_level: (2, 2, m_next, n_next)."""
    m_prev, n_prev = V_prev.shape[2:]
    yn, xn = np.mgrid[0:m_next, 0:n_next]
    odd = (xn % 2 != 0) | (yn % 2 != 0)
    yci, xci = np.minimum(yn // 2, m_prev - 1), np.minimum(xn // 2, n_prev - 1)
    out = np.empty((2, 2, m_next, n_next))
    for i in range(2):
        for k in range(2):
            out[i, k] = 2.0 * np.where(odd, interpolate(V_prev[i, k], xn / 2.0, yn / 2.0), V_prev[i, k][yci, xci])
    return out


def level_shapes(m, n, n_levels):
    out = [(m, n)]
    for _ in range(1, n_levels):
        out.append((int(out[-1][0] / 2), int(out[-1][1] / 2)))
    return out


def compute_advection_field(R, lam, num_iter, n_levels, c_sum="sequential", jacobi=False):
    """_compute_advection_field on the scaled frames R (2, m, n): (V (2, 2, m, n), GAMMA (2, m, n))."""
    pyr = [pyramid(R[0], n_levels), pyramid(R[1], n_levels)]
    V = np.zeros((2, 2) + pyr[0][-1].shape)
    step = sweep_jacobi if jacobi else sweep
    for i in range(n_levels - 1, -1, -1):
        Ri = np.stack([pyr[0][i], pyr[1][i]])
        G = np.stack([gradients(Ri[0]), gradients(Ri[1])])
        for _ in range(num_iter):
            step(V, consistency_maps(V, c_sum), Ri, G, lam)
        if i > 0:
            V = next_level(V, *pyr[0][i - 1].shape)
    return V, consistency_maps(V, c_sum)


def proesmans(input_images, lam=50.0, num_iter=100, num_levels=6, filter_std=0.0, full_output=False,
              c_sum="sequential", jacobi=False):
    from scipy.ndimage import gaussian_filter

    im = scale_frames(np.asarray(input_images))
    if filter_std > 0.0:
        im[0] = gaussian_filter(im[0], filter_std)
        im[1] = gaussian_filter(im[1], filter_std)
    V, GAMMA = compute_advection_field(im, lam, num_iter, num_levels, c_sum, jacobi)
    return (V, GAMMA) if full_output else V[0]


def recipe_frames(m, n, seed):
    """The test frames: smoothed noise, thresholded, and the same field shifted by (1.7, -2.3) pixels."""
    from scipy.ndimage import gaussian_filter, shift

    base = gaussian_filter(np.random.default_rng(seed).random((m + 20, n + 20)), 3.0)
    base = np.where(base > 0.5, base - 0.5, 0)
    moved = shift(base, (1.7, -2.3), order=1)
    return np.stack([base[10:10 + m, 10:10 + n], moved[10:10 + m, 10:10 + n]])


def golden_case(z, name):
    """A case of tests/golden/proesmans_reference.npz (tools/make_golden_proesmans.py): the frames in the case's dtype
    (rebuilt from the recipe and held to the stored digest where the file holds no frames), the keywords, the stride of
    the stored planes, the reference's planes and the exact-mode restatement's."""
    import hashlib
    import json

    kw = json.loads(str(z[name + "__kwargs"]))
    m, n, seed, dtype = kw.pop("m"), kw.pop("n"), kw.pop("seed"), kw.pop("dtype")
    kw.pop("device")
    if name + "__frames" in z.files:
        frames = z[name + "__frames"]
    else:
        frames = recipe_frames(m, n, seed).astype(dtype)
        sha = hashlib.sha256(np.ascontiguousarray(frames).tobytes()).hexdigest()
        assert sha == str(z[name + "__frames_sha256"]), "%s: the recipe no longer gives the golden's frames" % name
    ref_V, ref_G = z[name + "__ref_V"], z[name + "__ref_G"]
    return dict(frames=frames, kw=kw, stride=int(z[name + "__stride"]), ref_V=ref_V, ref_G=ref_G,
                exact_V=ref_V + z[name + "__exact_dV"], exact_G=ref_G + z[name + "__exact_dG"])
