"""NumPy float64 reference of the statistical inefficiency and of the block bootstrap of MBAR - TEST INFRASTRUCTURE ONLY.

It materialises the N x K matrix of window weights (tests/mbar_newton_ref.py, tests/mbar_ref.py) and knows nothing of the
library.  A replicate b weights frame n by an integer multiplicity m_bn and solves sum_n m_bn W_nk(f_b) = 1 with
W_nk(f) = exp(f_k - u_kn - L_n(f)), L_n(f) = ln sum_j N_j exp(f_j - u_jn): the counts N_j stay the windows' own, a
window's multiplicities sum to N_k.  The solve is a full Newton iteration per replicate with the replicate's own Hessian
(vectorised over the replicates), not the library's chord iteration.
"""

from __future__ import annotations

import numpy as np

from tests import mbar_newton_ref as NR
from tests import mbar_ref as R


# ---- statistical inefficiency ------------------------------------------------------------------------------------------
def autocorr(x, t):
    """C(t) of the definition, as plain loops."""
    T = len(x)
    mu = sum(float(a) for a in x) / T
    v = sum((float(a) - mu) ** 2 for a in x) / T
    acc = 0.0
    for i in range(T - t):
        acc += (float(x[i]) - mu) * (float(x[i + t]) - mu)
    return acc / ((T - t) * v)


def stat_ineff_loops(x, mintime=3):
    """g = max(1, 1 + 2 sum_{t=1}^{t*-1} C(t) (1 - t / T)), t* the first t > mintime with C(t) <= 0, T - 1 if none; 1 for
    T <= 2 or a constant series.  Plain loops: for short series."""
    T = len(x)
    if T <= 2 or np.ptp(np.asarray(x, dtype=np.float64)) == 0.0:
        return 1.0
    g, t = 1.0, 1
    while t < T - 1:
        c = autocorr(x, t)
        if c <= 0.0 and t > mintime:
            break
        g += 2.0 * c * (1.0 - t / T)
        t += 1
    return max(g, 1.0)


def stat_ineff(x, mintime=3, return_tstar=False):
    """The same with the inner sum as a dot product: for long series."""
    x = np.asarray(x, dtype=np.float64)
    T = len(x)
    d = x - x.mean()
    v = (d * d).mean()
    if T <= 2 or v == 0.0:
        return (1.0, T - 1) if return_tstar else 1.0
    g, t = 1.0, 1
    while t < T - 1:
        c = float(d[:T - t] @ d[t:]) / ((T - t) * v)
        if c <= 0.0 and t > mintime:
            break
        g += 2.0 * c * (1.0 - t / T)
        t += 1
    return (max(g, 1.0), t) if return_tstar else max(g, 1.0)


def stat_ineff_set(x, n_k, mintime=3):
    """(K, E) for the segments of an (N, E) array."""
    x = np.asarray(x, dtype=np.float64)
    off = np.concatenate([[0], np.cumsum(n_k)])
    return np.array([[stat_ineff(x[off[k]:off[k + 1], e], mintime) for e in range(x.shape[1])] for k in range(len(n_k))])


def ar1(rng, phi, shape):
    """Stationary AR(1) series of unit variance along the last axis: g = (1 + phi) / (1 - phi)."""
    z = rng.standard_normal(shape)
    out = np.empty(shape)
    out[..., 0] = z[..., 0]
    s = np.sqrt(1.0 - phi * phi)
    for t in range(1, shape[-1]):
        out[..., t] = phi * out[..., t - 1] + s * z[..., t]
    return out


def correlated_gaussian_case(K, n_per, phi, seed, k0=2.0, k=8.0, spacing_sigma=1.5):
    """``mbar_ref.gaussian_case`` with AR(1) frames inside every window: the same exact marginals, frames correlated."""
    c = R.gaussian_case(K=K, n_per=n_per, k0=k0, k=k, spacing_sigma=spacing_sigma, seed=seed)
    mean = c["k"] * c["c"] / (c["k0"] + c["k"])
    z = ar1(np.random.default_rng(10_000 + seed), phi, (K, n_per))
    c["xi"] = np.ascontiguousarray((mean[:, None] + c["sigma"] * z).reshape(-1, 1))
    return c


# ---- resampling ----------------------------------------------------------------------------------------------------------
def multiplicities(n_k, starts, lengths):
    """(n_boot, N) int64 rebuilt from the starts, block by block and frame by frame."""
    off = np.concatenate([[0], np.cumsum(n_k)])
    n_boot = starts[0].shape[0]
    m = np.zeros((n_boot, int(off[-1])), dtype=np.int64)
    for k in range(len(n_k)):
        for b in range(n_boot):
            for j, length in enumerate(lengths[k]):
                s = int(starts[k][b, j])
                assert 0 <= s and s + length <= n_k[k]
                for i in range(int(length)):
                    m[b, off[k] + s + i] += 1
    return m


# ---- the weighted sums and the weighted solve ------------------------------------------------------------------------------
def colsums(u, n_k, f_hat, delta, m):
    """(B, K): s_bk = sum_n m_bn W_nk(f_hat + delta_b)."""
    return np.stack([np.asarray(m[b], dtype=np.float64) @ NR.weights_matrix(u, n_k, f_hat + delta[b]) for b in range(len(delta))])


def binned(u, n_k, f_hat, delta, m, segments, v=None, shift=0.0):
    """(B, n_seg, max(E, 1)): sum over a segment's frames of m_bn v_ne exp(-L_n(f_hat + delta_b) - shift)."""
    N = u.shape[1]
    v = np.ones((N, 1)) if v is None else np.asarray(v, dtype=np.float64).reshape(N, -1)
    out = np.zeros((len(delta), len(segments), v.shape[1]))
    for b in range(len(delta)):
        a = np.asarray(m[b], dtype=np.float64) * np.exp(R.log_weights(u, n_k, f_hat + delta[b]) - shift)
        for i, seg in enumerate(segments):
            seg = np.asarray(seg, dtype=np.int64)
            out[b, i] = (a[seg, None] * v[seg]).sum(axis=0)
    return out


def weighted_residual(u, n_k, f, m):
    """max_k |f' - f| of one weighted fixed-point map f'_k = f_k - ln s_k, re-gauged, at ``f`` (K,)."""
    ln_s = np.log(np.asarray(m, dtype=np.float64) @ NR.weights_matrix(u, n_k, f))
    return np.abs(ln_s - ln_s[0]).max()


def weighted_newton(u, n_k, m, tol=1e-12, max_iter=50, f0=None):
    """(B, K): every replicate's f_b with f_b0 = 0 by guarded Newton iterations, each replicate with its own Hessian
    H_b = [diag(N_k s_bk) - N_i N_j (W^T diag(m_b) W)_ij] / N and gradient g_bk = N_k (s_bk - 1) / N, against the
    self-consistent candidate; until max_k |ln s_bk - ln s_b0| <= tol for all."""
    u, m = np.asarray(u, dtype=np.float64), np.asarray(m, dtype=np.float64)
    n = np.asarray(n_k, dtype=np.float64)
    B, K, total = m.shape[0], len(n), n.sum()
    ln_n = np.log(n)
    f = np.zeros((B, K)) if f0 is None else np.broadcast_to(np.asarray(f0, dtype=np.float64) - np.asarray(f0)[..., :1], (B, K)).copy()

    def weights(f):  # (B, N, K)
        a = (ln_n + f)[:, None, :] - u.T[None, :, :]
        top = a.max(axis=2, keepdims=True)
        L = top + np.log(np.exp(a - top).sum(axis=2, keepdims=True))
        return np.exp(f[:, None, :] - u.T[None, :, :] - L)

    def sums(f):
        W = weights(f)
        return W, np.einsum("bn,bnk->bk", m, W)

    W, s = sums(f)
    for _ in range(max_iter):
        ln_s = np.log(s)
        if (np.abs(ln_s - ln_s[:, :1]).max(axis=1) <= tol).all():
            return f
        grad = n[None, :] * (s - 1.0) / total
        fixed = f - ln_s + ln_s[:, :1]
        newton = fixed
        if K > 1:
            G = np.einsum("bn,bni,bnj->bij", m, W, W)
            H = (np.einsum("k,bk,kj->bkj", n, s, np.eye(K)) - n[None, :, None] * n[None, None, :] * G) / total
            newton = f.copy()
            newton[:, 1:] -= np.linalg.solve(H[:, 1:, 1:], grad[:, 1:, None])[:, :, 0]
        W_n, s_n = sums(newton)
        W_f, s_f = sums(fixed)
        better = np.linalg.norm(n * (s_f - 1.0), axis=1) < np.linalg.norm(n * (s_n - 1.0), axis=1)
        f = np.where(better[:, None], fixed, newton)
        s = np.where(better[:, None], s_f, s_n)
        W = np.where(better[:, None, None], W_f, W_n)
    raise RuntimeError("mbar_boot_ref.weighted_newton: not converged")


# ---- statistics over replicates ----------------------------------------------------------------------------------------------
def boot_f_sigma(boot_f):
    """(K, K): sample standard deviation (ddof = 1) of f_i - f_j over the replicates."""
    d = boot_f[:, :, None] - boot_f[:, None, :]
    return d.std(axis=0, ddof=1)


def boot_profiles(u, n_k, boot_f, m, x, edges, kT, weights=None):
    """(B, bins): every replicate's profile, +inf where a bin is empty in the replicate."""
    out = []
    for b in range(len(boot_f)):
        a = np.asarray(m[b], dtype=np.float64) * (1.0 if weights is None else np.asarray(weights, dtype=np.float64))
        lw = R.log_weights(u, n_k, boot_f[b])
        e = a * np.exp(lw - lw.max())
        row = np.full(len(edges) - 1, np.inf)
        for i in range(len(edges) - 1):
            s = e[(x >= edges[i]) & (x < edges[i + 1])].sum()
            if s > 0.0:
                row[i] = -kT * (np.log(s) - np.log(e.sum()))
        out.append(row)
    return np.asarray(out)


def profile_sigma(F, ref):
    """(bins,): standard deviation over the replicates of F_b - F_ref, a replicate counted where both bins are occupied in it;
    NaN where that is fewer than two."""
    out = np.full(F.shape[1], np.nan)
    for i in range(F.shape[1]):
        both = np.isfinite(F[:, i]) & np.isfinite(F[:, ref])
        if both.sum() >= 2:
            out[i] = np.std(F[both, i] - F[both, ref], ddof=1)
    return out


def profile_interval(F, level=0.95):
    """(2, bins): the percentile bounds over the replicates in which the bin is occupied; NaN where fewer than two."""
    out = np.full((2, F.shape[1]), np.nan)
    for i in range(F.shape[1]):
        col = F[np.isfinite(F[:, i]), i]
        if len(col) >= 2:
            out[:, i] = np.percentile(col, [50.0 * (1.0 - level), 50.0 * (1.0 + level)])
    return out


def expect_sigma(u, n_k, boot_f, m, values, weights=None):
    """Standard deviation over the replicates of sum_n m_bn w_n e^{lw_bn} A_n / sum_n m_bn w_n e^{lw_bn}; values (N,) or (N, E)."""
    vals = []
    for b in range(len(boot_f)):
        a = np.asarray(m[b], dtype=np.float64) * (1.0 if weights is None else np.asarray(weights, dtype=np.float64))
        vals.append(R.expect(R.log_weights(u, n_k, boot_f[b]), values, weights=a))
    return np.std(np.asarray(vals), axis=0, ddof=1)
