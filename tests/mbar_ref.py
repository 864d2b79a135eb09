"""NumPy float64 reference of MBAR and of the PMF over its weights - TEST INFRASTRUCTURE ONLY.

Written from the definitions with ``scipy.special.logsumexp``; it materialises the K x N bias matrix
and knows nothing of the library.  Window tables are (K, P, 4) = {kind, k, init, rate}, kind 0 umbrella, 1 constant force.

``gaussian_case`` is the analytic case: a base potential 1/2 k0 xi^2 under umbrellas 1/2 k (xi - c_k)^2 samples exact
Gaussians of mean k c_k / (k0 + k) and variance kT / (k0 + k), with f_k - f_0 = 1/2 beta k0 k / (k0 + k) (c_k^2 - c_0^2) and
F(xi) = 1/2 k0 xi^2.
"""

from __future__ import annotations

import numpy as np
from scipy.special import logsumexp


def bias(table, xi, kT):
    """(K, N) reduced bias b_k(n) = beta sum_p U_kp(xi_np)."""
    table, xi = np.asarray(table, dtype=np.float64), np.asarray(xi, dtype=np.float64)
    K, P, _ = table.shape
    u = np.zeros((K, xi.shape[0]))
    for k in range(K):
        for p in range(P):
            kind, kk, init, _ = table[k, p]
            u[k] += kk * xi[:, p] if kind == 1 else 0.5 * kk * (xi[:, p] - init) ** 2
    return u / kT


def iterate(u, n_k, f):
    """One iteration from f: (f' with f'_0 = 0, L (N,), t (K, N) the responsibilities at f)."""
    ln_n = np.log(np.asarray(n_k, dtype=np.float64))
    a = (ln_n + f)[:, None] - u
    L = logsumexp(a, axis=0)
    f_new = -logsumexp(-u - L[None, :], axis=1)
    return f_new - f_new[0], L, np.exp(a - L[None, :])


def solve(u, n_k, tol=1e-10, max_iter=200_000, f0=None):
    """-> (f, iterations, delta), from f0 (zeros where None)."""
    f = np.zeros(u.shape[0]) if f0 is None else np.asarray(f0, dtype=np.float64) - f0[0]
    for it in range(1, max_iter + 1):
        g, _, _ = iterate(u, n_k, f)
        d = np.abs(g - f).max()
        f = g
        if d <= tol:
            return f, it, d
    raise RuntimeError(f"mbar_ref.solve: not converged, delta {d}")


def log_weights(u, n_k, f):
    return -iterate(u, n_k, f)[1]


def expect(lw, values, weights=None):
    a = np.exp(lw - lw.max()) * (1.0 if weights is None else np.asarray(weights))
    v = np.asarray(values, dtype=np.float64)
    return (a.reshape(-1, *([1] * (v.ndim - 1))) * v).sum(0) / a.sum()


def n_eff(lw, weights=None):
    a = np.exp(lw - lw.max()) * (1.0 if weights is None else np.asarray(weights))
    return a.sum() ** 2 / (a * a).sum()


def pmf(lw, x, edges, kT, weights=None):
    """F_b = -kT [ln sum_{n in b} w_n e^{lw_n} - ln sum_n w_n e^{lw_n}]; +inf for an empty bin; x in [e_b, e_b+1)."""
    edges = np.asarray(edges, dtype=np.float64)
    lw = lw if weights is None else lw + np.log(np.asarray(weights, dtype=np.float64))
    total = logsumexp(lw)
    out = np.full(len(edges) - 1, np.inf)
    for b in range(len(edges) - 1):
        sel = (x >= edges[b]) & (x < edges[b + 1])
        if sel.any():
            out[b] = -kT * (logsumexp(lw[sel]) - total)
    return out


# ---- the analytic case ------------------------------------------------------------------------------------------------
def gaussian_case(K=8, n_per=400, k0=2.0, k=8.0, kT=1.0, spacing_sigma=1.5, seed=0, copies=1):
    """Exact samples of K windows (``copies`` replicas each, ``n_per`` frames per replica, pooled window-major): dict(xi (N, 1),
    table (K * copies, 1, 4), n_k, centres c (K,), f (K,) analytic, sigma, k0, k, kT)."""
    sigma = np.sqrt(kT / (k0 + k))
    mean_step = spacing_sigma * sigma            # the windows' means are spacing_sigma standard deviations apart
    c = (np.arange(K) - 0.5 * (K - 1)) * mean_step * (k0 + k) / k  # mean = k c / (k0 + k); the windows straddle xi = 0
    rng = np.random.default_rng(seed)
    cc = np.repeat(c, copies)
    xi = (k * cc / (k0 + k))[:, None] + sigma * rng.standard_normal((K * copies, n_per))
    table = np.zeros((K * copies, 1, 4))
    table[:, 0, 1], table[:, 0, 2] = k, cc
    f = 0.5 / kT * k0 * k / (k0 + k) * (c**2 - c[0] ** 2)
    return dict(xi=xi.reshape(-1, 1), table=table, n_k=np.full(K * copies, n_per, dtype=np.int64), c=c, f=f, sigma=sigma, k0=k0, k=k, kT=kT,
                copies=copies)


def gaussian_pmf_error(case, edges, tol=1e-10):
    """(F_b - 1/2 k0 xi_b^2 with the mean over the occupied bins removed, occupied (B,) bool) of the reference's PMF of a case;
    the solve starts from the analytic f."""
    u = bias(case["table"], case["xi"], case["kT"])
    f, _, _ = solve(u, case["n_k"], tol=tol, f0=case["f"])
    F = pmf(log_weights(u, case["n_k"], f), case["xi"][:, 0], edges, case["kT"])
    centres = 0.5 * (np.asarray(edges)[1:] + np.asarray(edges)[:-1])
    occ = np.isfinite(F)
    err = np.where(occ, F - 0.5 * case["k0"] * centres**2, 0.0)
    return err - err[occ].mean() * occ, occ


# ---- the layout of the end-to-end test (tests/test_gpu_mbar.py), shared with the CPU check of its bins -----------------
E2E = dict(K=8, copies=8, rows=50, k0=100.0, k=500.0, kT=2.5, spacing_sigma=1.5)  # kJ/mol, nm: sigma = 0.0645 nm
E2E_SEEDS = 32


def e2e_edges():
    """24 bins of half a standard deviation on [-6 sigma, 6 sigma]; the windows' means span [-5.25 sigma, 5.25 sigma]."""
    sigma = np.sqrt(E2E["kT"] / (E2E["k0"] + E2E["k"]))
    return np.linspace(-6.0 * sigma, 6.0 * sigma, 25)


def e2e_case(seed):
    """Exact Gaussian samples with the counts of the end-to-end run.  The eight copies of a window share its bias, so they are
    one state of 8 x rows frames: the MBAR equations of the 64-state layout reduce to these eight, weight for weight."""
    e = E2E
    return gaussian_case(K=e["K"], n_per=e["copies"] * e["rows"], k0=e["k0"], k=e["k"], kT=e["kT"], spacing_sigma=e["spacing_sigma"], seed=seed)


_E2E_CACHE = {}


def e2e_reference():
    """dict(sigma (B,) standard deviation over E2E_SEEDS draws of the reference PMF's error per bin, kJ/mol; use (B,) bool: the
    bins occupied in every draw; inside (B,) bool: the bins whose centre lies within the range of the windows' means; edges,
    centres).  Computed once per process.  The solves stop at 1e-8, seven orders below the scatter they measure."""
    if not _E2E_CACHE:
        edges = e2e_edges()
        errs, occ = zip(*(gaussian_pmf_error(e2e_case(seed), edges, tol=1e-8) for seed in range(E2E_SEEDS)))
        use = np.all(occ, axis=0)
        c = e2e_case(0)
        means = c["k"] * c["c"] / (c["k0"] + c["k"])
        centres = 0.5 * (edges[1:] + edges[:-1])
        _E2E_CACHE.update(sigma=np.std(np.asarray(errs), axis=0, ddof=1), use=use, inside=(centres >= means[0]) & (centres <= means[-1]),
                          edges=edges, centres=centres)
    return _E2E_CACHE
