"""BPS motion perturbation (pysteps/noise/motion.py) on the oracle side of the member-advection tests."""

import numpy as np


def perturbators(n, seed):
    rng = np.random.default_rng(seed)
    # parameters of pysteps.noise.motion.initialize_bps (defaults p_par/p_perp of the reference)
    return [dict(eps_par=rng.laplace(scale=1 / np.sqrt(2)), eps_perp=rng.laplace(scale=1 / np.sqrt(2)),
                 p_par=(10.88, 0.23, -7.68), p_perp=(5.76, 0.31, -2.72), vsf=60.0 / (5.0 * 1.0)) for _ in range(n)]


def generate_bps(V, p, t):
    """NumPy restatement of noise/motion.py:127-131,146-180 for the oracle side."""
    N = np.linalg.norm(V, axis=0)
    Vn = np.where(N > 1e-12, V / np.where(N > 1e-12, N, 1.0), 0.0)
    Vp = np.stack([-Vn[1], Vn[0]])
    g_par = p["p_par"][0] * pow(t, p["p_par"][1]) + p["p_par"][2]
    g_perp = p["p_perp"][0] * pow(t, p["p_perp"][1]) + p["p_perp"][2]
    return (g_par * p["eps_par"] * Vn + g_perp * p["eps_perp"] * Vp) / p["vsf"]
