"""NumPy float64 reference of the MBAR Gram matrix, the guarded Newton solve and the asymptotic error bars - TEST
INFRASTRUCTURE ONLY.

It materialises the N x K matrix of window weights W_nk = exp(f_k - b_k(n) - L_n) (tests/mbar_ref.py supplies b and L) and
knows nothing of the library.  ``theta_direct`` is the N x N definition of the covariance (Shirts and Chodera 2008, eq. 8),
``theta_eig`` the route through the Gram matrix alone that the library takes; ``pmf_sigma`` and ``expect_sigma`` stand on the
former.
"""

from __future__ import annotations

import numpy as np

from tests import mbar_ref as R


def weights_matrix(u, n_k, f):
    """(N, K): W_nk = exp(f_k - u_kn - L_n), L_n = ln sum_j N_j exp(f_j - u_jn); sum_k N_k W_nk = 1 for every frame."""
    _, L, _ = R.iterate(u, n_k, np.asarray(f, dtype=np.float64))
    return np.exp(np.asarray(f)[None, :] - u.T - L[:, None])


def gram(u, n_k, f):
    """(G (K, K) = W^T W, s (K,) = column sums of W)."""
    W = weights_matrix(u, n_k, f)
    return W.T @ W, W.sum(axis=0)


def segment_moments(u, n_k, f, segments, v=None):
    """(n_seg, K): sum over the frames of each segment (an index array) of v_n W_nk."""
    W = weights_matrix(u, n_k, f)
    if v is not None:
        W = W * np.asarray(v, dtype=np.float64)[:, None]
    return np.stack([W[np.asarray(seg, dtype=np.int64)].sum(axis=0) for seg in segments])


def newton(u, n_k, tol=1e-10, max_iter=100, f0=None):
    """The guarded Newton iteration in the gauge f_0 = 0 -> (f, iterations, delta).  Per iteration the Newton candidate
    f - H^-1 g on the windows 1 ... K - 1 (g_k = N_k (s_k - 1) / N, H = [diag(N_k s_k) - N_i N_j G_ij] / N) and the
    self-consistent candidate f - ln s, re-gauged; the one with the smaller gradient norm is kept.  delta is max |f' - f| of
    one fixed-point map at the accepted point.  Starts from f0, or from zeros after two fixed-point iterations."""
    n = np.asarray(n_k, dtype=np.float64)
    total, K = n.sum(), len(n)
    if f0 is None:
        f = np.zeros(K)
        for _ in range(2):
            f = R.iterate(u, n_k, f)[0]
    else:
        f = np.asarray(f0, dtype=np.float64) - f0[0]
    G, s = gram(u, n_k, f)
    for it in range(1, max_iter + 1):
        grad = n * (s - 1.0) / total
        hess = (np.diag(n * s) - (n[:, None] * n[None, :]) * G) / total
        cands = [f - np.log(s) + np.log(s[0])]
        if K > 1:
            cands.insert(0, f - np.concatenate([[0.0], np.linalg.solve(hess[1:, 1:], grad[1:])]))
        scored = []
        for c in cands:
            G_c, s_c = gram(u, n_k, c)
            scored.append((np.linalg.norm(n * (s_c - 1.0) / total), c, G_c, s_c))
        _, f, G, s = min(scored, key=lambda t: t[0])
        d = np.abs(np.log(s) - np.log(s[0])).max()
        if d <= tol:
            return f, it, d
    raise RuntimeError(f"mbar_newton_ref.newton: not converged, delta {d}")


def augmented(W, columns):
    """(N, K + A): W followed by the extra columns, each normalised to sum 1."""
    cols = [np.asarray(c, dtype=np.float64) / np.sum(c) for c in columns]
    return np.concatenate([W] + [c[:, None] for c in cols], axis=1) if cols else W


def theta_direct(W, n):
    """Theta = W^T (I - W N W^T)^+ W by the N x N definition (N <= 600); ``n`` the columns' counts, 0 for an augmented one."""
    W, n = np.asarray(W), np.asarray(n, dtype=np.float64)
    assert W.shape[0] <= 600
    return W.T @ np.linalg.pinv(np.eye(W.shape[0]) - (W * n[None, :]) @ W.T) @ W


def theta_eig(G, n):
    """Theta from G = W^T W alone: G = V S^2 V^T, M = I - S V^T N V S with the one null vector y = S V^T n,
    M^+ = (M + yy^T)^-1 - yy^T (y normalised), Theta = V S M^+ S V^T."""
    n = np.asarray(n, dtype=np.float64)
    lam, V = np.linalg.eigh(0.5 * (G + G.T))
    VS = V * np.sqrt(np.clip(lam, 0.0, None))[None, :]
    M = np.eye(len(lam)) - VS.T @ (n[:, None] * VS)
    y = VS.T @ n
    y /= np.linalg.norm(y)
    return VS @ (np.linalg.inv(M + np.outer(y, y)) - np.outer(y, y)) @ VS.T


def sigma(theta):
    """(A, A): standard deviation of the difference of every two columns' log normalisation constants."""
    d = np.diag(theta)
    return np.sqrt(np.clip(d[:, None] + d[None, :] - 2.0 * theta, 0.0, None))


def bin_columns(lw, x, edges):
    """(the occupied bins' indices, their columns e^{lw} restricted to the bin) for x in [e_b, e_b+1)."""
    e = np.exp(lw - lw.max())
    occ, cols = [], []
    for b in range(len(edges) - 1):
        sel = (x >= edges[b]) & (x < edges[b + 1])
        if sel.any():
            occ.append(b), cols.append(np.where(sel, e, 0.0))
    return np.asarray(occ), cols


def pmf_gram(u, n_k, f, x, edges):
    """(augmented Gram matrix of the windows and the occupied bins' columns, counts, occupied bins)."""
    W = weights_matrix(u, n_k, f)
    occ, cols = bin_columns(R.log_weights(u, n_k, f), x, edges)
    Wa = augmented(W, cols)
    return Wa.T @ Wa, np.concatenate([np.asarray(n_k, dtype=np.float64), np.zeros(len(occ))]), occ


def pmf_sigma_from_theta(theta, K, occ, n_bins, kT, reference="min", F=None):
    """(B,) sigma(F_b - F_ref); NaN at empty bins; ``reference`` a bin or "min" (the occupied bin of lowest ``F``)."""
    ref = int(occ[np.argmin(F[occ])]) if reference == "min" else int(reference)
    out = np.full(n_bins, np.nan)
    out[occ] = kT * sigma(theta)[K:, K + int(np.searchsorted(occ, ref))]
    return out


def pmf_sigma(u, n_k, f, x, edges, kT, reference="min"):
    """(B,) kJ/mol by ``theta_direct``."""
    W = weights_matrix(u, n_k, f)
    lw = R.log_weights(u, n_k, f)
    occ, cols = bin_columns(lw, x, edges)
    n = np.concatenate([np.asarray(n_k, dtype=np.float64), np.zeros(len(occ))])
    return pmf_sigma_from_theta(theta_direct(augmented(W, cols), n), len(n_k), occ, len(edges) - 1, kT, reference, R.pmf(lw, x, edges, kT))


def expect_columns(lw, values):
    """(the two columns of one observable, <A'>) with A' = A - min A + 1."""
    e = np.exp(lw - lw.max())
    shifted = np.asarray(values, dtype=np.float64) - np.min(values) + 1.0
    return [e * shifted, e], float((e * shifted).sum() / e.sum())


def expect_sigma(u, n_k, f, values):
    """sigma of <A> for values (N,) by ``theta_direct``: <A'> sqrt(Theta_AA + Theta_aa - 2 Theta_Aa)."""
    W = weights_matrix(u, n_k, f)
    cols, mean = expect_columns(R.log_weights(u, n_k, f), values)
    K = len(n_k)
    theta = theta_direct(augmented(W, cols), np.concatenate([np.asarray(n_k, dtype=np.float64), np.zeros(2)]))
    return mean * sigma(theta)[K, K + 1]
