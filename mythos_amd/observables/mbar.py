"""Umbrella windows to a free-energy profile: the binless multistate estimator MBAR (the binless form of WHAM) on the GPU,
and a PMF observable over its per-frame weights that is differentiable in DiffTRe's weights (mythos_amd/csrc/mbar.hip,
``mythos_mbar_*``; definitions in DESIGN section 3.5o).

    windows = np.linspace(0.0, 2.0, 8)
    rs = MartiniRestraints(pulls=[PullCoordinate(..., k=1000.0, init=windows)])
    out = HipMartiniSimulator(..., temperatures=[310.0] * 8, restraints=rs).run(seed=1)
    xi = out.state["pull"]                                   # (rows, 8, 1) float64 on the GPU

    res = mbar_umbrella(xi, rs, kT=KB * 310.0)               # MbarResult: f (K,), log_weights (N,), iterations, delta
    traj = SimulatorTrajectory.concat(out.observables)       # frame n = r * rows + row: the order of res.log_weights
    mean = res.expect(observable(traj))                      # the unbiased average; expect(values, weights) under DiffTRe

    pmf = UmbrellaPMF(restraints=rs, coordinate=0, kT=KB * 310.0, edges=np.linspace(0.0, 2.0, 41))
    pmf.fit(xi)                                              # once per stored trajectory: solves MBAR, sorts by bin
    F = pmf(weights)                                         # (B,) kJ/mol on the GPU, inside a DiffTReObjective loss

Frames n = 0 ... N - 1 are pooled from K windows, window k contributed N_k >= 1 of them.  b_k(n) is the reduced bias of
window k at frame n: for a ``MartiniRestraints`` set, beta times the sum over ALL its pull coordinates of
1/2 k_kp (xi_np - init_kp)^2 (``umbrella``) or k_kp xi_np (``constant-force``), with ``init`` and ``k`` of replica k.  MBAR solves

    L_n = ln sum_j N_j exp(f_j - b_j(n)),        f_k = -ln sum_n exp(-b_k(n) - L_n),        f_0 = 0

by fixed-point iteration; lw_n = -L_n are the frames' unbiasing log-weights, defined up to a constant.  With DiffTRe
weights w_n over the same frames, <O> = sum_n w_n e^{lw_n} O_n / sum_n w_n e^{lw_n}.  The bias does not depend on the
parameters that are optimised, so the f_k solved once at the reference parameters stay valid importance weights.  The PMF
over coordinate p with bin edges e_0 < ... < e_B is

    F_b = -kT [ln sum_{n: xi_np in [e_b, e_b+1)} w_n e^{lw_n} - ln sum_n w_n e^{lw_n}]      (kJ/mol; +inf for an empty bin)

and ``jacobian="distance"`` adds kT (d - 1) ln xi_b at the bin centres, d the number of axes in the coordinate's ``dim``.

``mbar(u_kn, n_k)`` is the general entry: any (K, N) matrix of reduced energies on the GPU, a temperature ladder's
beta_k (U_n + p V_n) for instance.  The host queues ``check_every`` iterations without a synchronisation and then reads
one word, max_k |f' - f|; the solve stops when it is at most ``tol`` and raises ``MbarNotConverged`` after ``max_iter``.

``solver="newton"`` solves the same equations by a guarded Newton iteration in the gauge f_0 = 0.  With the window weights
W_nk = exp(f_k - b_k(n) - L_n), s_k = sum_n W_nk and the Gram matrix G = W^T W (``mythos_mbar_gram``: W is formed on the fly,
never stored), the gradient is g_k = N_k (s_k - 1) / N and the Hessian H = [diag(N_k s_k) - N_i N_j G_ij] / N; the K - 1
linear solve runs on the host.  Every iteration forms the Newton candidate and the self-consistent candidate f - ln s,
evaluates s at both (``mythos_mbar_segment_moments``) and keeps the one with the smaller |g|; it starts from zeros after two
fixed-point iterations.  ``delta`` is max_k |f' - f| of one fixed-point map at the accepted point, so ``tol``,
``MbarNotConverged`` and ``MbarResult.delta`` read the same for both solvers; ``iterations`` counts Newton iterations and
``check_every`` is ignored.  The default stays "fixed-point".

``uncertainties=True`` fills ``MbarResult.theta``, the estimator's asymptotic covariance (Shirts and Chodera, J. Chem. Phys.
129, 124105, 2008, eq. 8 and D), computed from G alone (``_theta``): ``f_error()`` is sigma(f_i - f_j),
``UmbrellaPMF.uncertainty()`` sigma(F_b - F_ref) of the unweighted profile and ``UmbrellaPMF.expect_error(values)`` sigma of
``result.expect(values)``.  The error bars hold at the reference parameters (``weights=None``) and treat the frames as
independent: correlated frames make them too small by the square root of the statistical inefficiency.

Not built: error bars under DiffTRe weights, a statistical-inefficiency correction, bootstrap; states with N_k = 0, moving
windows (``rate``), 2-D profiles.
"""

from __future__ import annotations

import ctypes as C
import dataclasses as dc
import math

import numpy as np
import torch

from mythos_amd import _lib

SOLVERS = ("fixed-point", "newton")
ROW = 4  # kMbarRow of csrc/mbar_checks.h: kind (0 umbrella, 1 constant force), k, init, rate
_I64P = C.POINTER(C.c_int64)


class MbarNotConverged(RuntimeError):
    """The solve did not reach ``tol`` within ``max_iter`` iterations (of either solver); ``delta`` is the last max |f' - f|."""

    def __init__(self, message: str, delta: float, iterations: int):
        super().__init__(message)
        self.delta, self.iterations = delta, iterations


def window_table(restraints, n_windows: int, topology=None) -> np.ndarray:
    """(K, P, 4) float64 {kind, k, init, rate} of every window and pull coordinate of a ``MartiniRestraints`` set, window k
    being replica k of ``restraints.lower`` (per-replica ``init`` and ``k``)."""
    if not len(restraints.pulls):
        raise ValueError("the restraint set has no pull coordinate: nothing biases xi")
    low = restraints.lower(topology=topology, n_rep=int(n_windows))
    table = np.zeros((int(n_windows), len(restraints.pulls), ROW))
    table[:, :, 0] = (low["p_flags"] & 1)[None, :]
    table[:, :, 1:4] = low["p_param"][:, :, 0:3]
    return np.ascontiguousarray(table)


def check(n_k, table=None, kT=None, xi=None, edges=None, n_frames=None) -> None:
    """What the library refuses, without a device (mythos_mbar_check): raises ValueError with its message.  ``table`` (K, P, 4),
    ``kT`` scalar or (K,), ``xi`` (N, P) on the host, ``edges`` (B + 1,); each may be None."""
    c_ = lambda a, dt=np.float64: None if a is None else np.ascontiguousarray(a, dtype=dt)  # noqa: E731
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    n_k = c_(np.atleast_1d(n_k), np.int64)
    K = int(n_k.shape[0])
    table, xi, edges = c_(table), c_(xi), c_(edges)
    if kT is not None:
        kT = c_(np.broadcast_to(np.asarray(kT, dtype=np.float64), (K,)) if np.ndim(kT) == 0 else kT)
        if kT.shape != (K,):
            raise ValueError(f"kT must be a scalar or hold {K} values, one per window")
    P = int(table.shape[1]) if table is not None else (int(xi.shape[1]) if xi is not None and xi.ndim == 2 else 0)
    if table is not None and table.shape != (K, P, ROW):
        raise ValueError(f"the window table must have shape ({K}, P, {ROW})")
    N = int(n_frames) if n_frames is not None else (int(xi.shape[0]) if xi is not None else int(n_k.sum()))
    if xi is not None and xi.shape != (N, P):
        raise ValueError(f"xi must have shape ({N}, {P})")
    _lib.check(_lib.load().mythos_mbar_check(K, N, P, dp(table), dp(kT), n_k.ctypes.data_as(_I64P), dp(xi),
                                             0 if edges is None else int(edges.shape[0]), dp(edges)), "mbar_check")


class _MbarPlan(_lib.Handle):
    """mythos_mbar_t: one MBAR problem of N frames and K windows on one device, with the tensors the library borrows.
    Private: ``mbar``, ``mbar_umbrella`` and ``UmbrellaPMF`` are the interface (tests/test_gpu_api.py lists the public owners
    of a handle; this one's close() is tested with the kernels' own tests)."""

    _destroy = "mythos_mbar_destroy"

    def __init__(self, n_frames: int, n_windows: int, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MythosHipError("MBAR is solved by the HIP library: the frames must live on a GPU (mythos_amd has no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.N, self.K = int(n_frames), int(n_windows)
        self._borrowed = self._n_k = None
        super().__init__("mythos_mbar_create", self.N, self.K, self.device.index)

    def close(self):
        super().close()
        self._borrowed = None

    def _ours(self, t: torch.Tensor, shape: tuple, what: str) -> None:
        """The kernels index these tensors by N, K and P alone: a tensor of another size, type or device is refused here."""
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == self.device and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous float64 tensor of shape {shape} on {self.device}")

    def set_windows(self, table: np.ndarray, kT: np.ndarray, n_k: np.ndarray, xi: torch.Tensor) -> None:
        table, kT, n_k = (np.ascontiguousarray(a, dtype=t) for a, t in ((table, np.float64), (kT, np.float64), (n_k, np.int64)))
        if table.ndim != 3 or table.shape[0] != self.K or table.shape[2] != ROW or kT.shape != (self.K,) or n_k.shape != (self.K,):
            raise ValueError(f"the window table must have shape ({self.K}, P, {ROW}), kT and n_k ({self.K},)")
        self._ours(xi, (self.N, int(table.shape[1])), "xi")
        _lib.check(self._lib.mythos_mbar_set_windows(self._h, int(table.shape[1]), table.ctypes.data_as(_lib.c_double_p),
                                                     kT.ctypes.data_as(_lib.c_double_p), n_k.ctypes.data_as(_I64P), _lib.ptr(xi)), "mbar_set_windows")
        self._borrowed, self._n_k = xi, n_k

    def set_matrix(self, u_kn: torch.Tensor, n_k: np.ndarray) -> None:
        n_k = np.ascontiguousarray(n_k, dtype=np.int64)
        if n_k.shape != (self.K,):
            raise ValueError(f"n_k must hold {self.K} counts")
        self._ours(u_kn, (self.K, self.N), "u_kn")
        _lib.check(self._lib.mythos_mbar_set_matrix(self._h, _lib.ptr(u_kn), n_k.ctypes.data_as(_I64P)), "mbar_set_matrix")
        self._borrowed, self._n_k = u_kn, n_k

    def iterate(self, f: torch.Tensor, n_iter: int, delta: torch.Tensor) -> None:
        """``n_iter`` iterations queued on the current stream: ``f`` (K,) advanced in place, ``delta`` (1,) the last max |f' - f|."""
        self._ours(f, (self.K,), "f"), self._ours(delta, (1,), "delta")
        _lib.check(self._lib.mythos_mbar_iterate(self._h, _lib.ptr(f), int(n_iter), _lib.ptr(delta), _lib.stream(self.device)), "mbar_iterate")

    def log_weights(self, f: torch.Tensor) -> torch.Tensor:
        self._ours(f, (self.K,), "f")
        lw = torch.empty(self.N, dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mythos_mbar_log_weights(self._h, _lib.ptr(f), _lib.ptr(lw), _lib.stream(self.device)), "mbar_log_weights")
        return lw

    def binned_sum(self, seg_start: torch.Tensor, order: torch.Tensor, lw: torch.Tensor, weights, shift: float) -> torch.Tensor:
        """(B + 1,): per bin the sum of weights[n] exp(lw[n] - shift) over its frames, then the same sum over all frames."""
        n_bins = int(seg_start.shape[0]) - 1
        self._ours(lw, (self.N,), "log_weights")
        if weights is not None:
            self._ours(weights, (self.N,), "weights")
        if order.dtype != torch.int64 or tuple(order.shape) != (self.N,) or seg_start.dtype != torch.int64 or order.device != self.device:
            raise ValueError("order must be int64 of shape (N,), seg_start int64 of shape (B + 1,), on the plan's device")
        out = torch.empty(n_bins + 1, dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mythos_mbar_binned_sum(self._h, n_bins, _lib.ptr(seg_start), _lib.ptr(order), _lib.ptr(lw), _lib.ptr(weights),
                                                    float(shift), _lib.ptr(out), _lib.stream(self.device)), "mbar_binned_sum")
        return out

    def gram(self, f: torch.Tensor, colsum: bool = True):
        """-> (G (K, K), s (K,) or None) at ``f``: G_ij = sum_n W_ni W_nj and s_k = sum_n W_nk of the window weights
        W_nk = exp(f_k - b_k(n) - L_n), queued on the current stream."""
        self._ours(f, (self.K,), "f")
        g = torch.empty(self.K, self.K, dtype=torch.float64, device=self.device)
        s = torch.empty(self.K, dtype=torch.float64, device=self.device) if colsum else None
        _lib.check(self._lib.mythos_mbar_gram(self._h, _lib.ptr(f), _lib.ptr(g), _lib.ptr(s), _lib.stream(self.device)), "mbar_gram")
        return g, s

    def segment_moments(self, f: torch.Tensor, seg_start=None, order=None, v=None) -> torch.Tensor:
        """(n_seg, K): sum over the frames n of a segment of v_n W_nk at ``f``; ``order`` (N,) and ``seg_start`` (n_seg + 1,)
        as for ``binned_sum``, or neither: one segment over all frames.  ``v`` (N,) or None for 1."""
        self._ours(f, (self.K,), "f")
        if v is not None:
            self._ours(v, (self.N,), "v")
        if (order is None) != (seg_start is None):
            raise ValueError("order and seg_start come together")
        n_seg = 1
        if order is not None:
            n_seg = int(seg_start.shape[0]) - 1
            if (order.dtype != torch.int64 or tuple(order.shape) != (self.N,) or seg_start.dtype != torch.int64 or seg_start.dim() != 1
                    or order.device != self.device or seg_start.device != self.device or not (order.is_contiguous() and seg_start.is_contiguous())):
                raise ValueError("order must be int64 of shape (N,), seg_start int64 of shape (n_seg + 1,), contiguous on the plan's device")
        out = torch.empty(max(n_seg, 0), self.K, dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mythos_mbar_segment_moments(self._h, _lib.ptr(f), n_seg, _lib.ptr(seg_start), _lib.ptr(order), _lib.ptr(v),
                                                         _lib.ptr(out), _lib.stream(self.device)), "mbar_segment_moments")
        return out

    def _newton(self, tol: float, max_iter: int, f0):
        """The guarded Newton iteration on the host, G and s from the device (module docstring) -> (f, iterations, delta)."""
        n = self._n_k.astype(np.float64)
        total, K = n.sum(), self.K
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=self.device)  # noqa: E731
        if f0 is None:
            start = torch.zeros(K, dtype=torch.float64, device=self.device)
            self.iterate(start, 2, torch.empty(1, dtype=torch.float64, device=self.device))
            f = start.cpu().numpy()
        else:
            f = np.array(torch.as_tensor(f0, dtype=torch.float64).reshape(K).cpu().numpy())
            f -= f[0]
        s, d = None, math.inf
        for it in range(1, max_iter + 1):
            g_d, s_d = self.gram(dev(f), colsum=s is None)  # s of an accepted candidate is already known
            G = g_d.cpu().numpy()
            if s is None:
                s = s_d.cpu().numpy()
            if not (np.isfinite(G).all() and np.isfinite(s).all() and (s > 0.0).all()):
                raise FloatingPointError(f"mbar: non-finite Gram matrix or column sums in Newton iteration {it}: windows without overlap?")
            grad = n * (s - 1.0) / total
            hess = (np.diag(n * s) - (n[:, None] * n[None, :]) * G) / total
            cands = [f - np.log(s) + np.log(s[0])]  # the self-consistent candidate: one fixed-point map, no launch
            if K > 1:
                try:
                    step = np.linalg.solve(hess[1:, 1:], grad[1:])
                except np.linalg.LinAlgError:
                    step = np.full(K - 1, np.nan)
                if np.isfinite(step).all():
                    cands.insert(0, f - np.concatenate([[0.0], step]))
            best = None
            for c in cands:
                s_c = self.segment_moments(dev(c))[0].cpu().numpy()
                if not (np.isfinite(s_c).all() and (s_c > 0.0).all()):
                    continue
                norm = float(np.linalg.norm(n * (s_c - 1.0) / total))
                if best is None or norm < best[0]:
                    best = (norm, c, s_c)
            if best is None:
                raise FloatingPointError(f"mbar: no finite candidate in Newton iteration {it}: windows without overlap?")
            _, f, s = best
            d = float(np.abs(np.log(s) - np.log(s[0])).max())  # max |f' - f| of one fixed-point map at the accepted point
            if d <= tol:
                return dev(f), it, d
        raise MbarNotConverged(f"mbar: not converged within max_iter = {max_iter}: after {max_iter} Newton iterations the last "
                               f"delta = max |f' - f| is {d:.3e}, tol = {tol:.3e}", d, max_iter)

    def solve(self, tol: float, max_iter: int, check_every: int, f0=None, solver: str = "fixed-point"):
        """-> (f (K,), iterations, delta).  ``"fixed-point"``: batches of ``check_every`` iterations (one batch of ``max_iter``
        where that is smaller), one device word read after each.  ``"newton"``: guarded Newton iterations, each one Gram
        launch, two moment launches and their read-backs (``check_every`` is ignored)."""
        tol, max_iter, check_every = float(tol), int(max_iter), int(check_every)
        if solver not in SOLVERS:
            raise ValueError(f"solver {solver!r}: expected one of {SOLVERS}")
        if not tol > 0.0 or max_iter < 1 or check_every < 1:
            raise ValueError("tol > 0, max_iter >= 1 and check_every >= 1 required")
        if solver == "newton":
            return self._newton(tol, max_iter, f0)
        f = torch.zeros(self.K, dtype=torch.float64, device=self.device)
        if f0 is not None:
            f.copy_(torch.as_tensor(f0, dtype=torch.float64).reshape(self.K))
        delta = torch.empty(1, dtype=torch.float64, device=self.device)
        batch, done, d = min(check_every, max_iter), 0, math.inf
        while done + batch <= max_iter:
            self.iterate(f, batch, delta)
            done += batch
            d = float(delta.item())
            if not math.isfinite(d):
                raise FloatingPointError(f"mbar: the iteration diverged after {done} iterations (delta = {d}): windows without overlap?")
            if d <= tol:
                return f, done, d
        raise MbarNotConverged(f"mbar: not converged within max_iter = {max_iter}: after {done} iterations the last "
                               f"delta = max |f' - f| is {d:.3e}, tol = {tol:.3e}", d, done)


def _combined(log_weights: torch.Tensor, weights) -> torch.Tensor:
    """w_n e^{lw_n - max lw}: the combined, unnormalised weights."""
    a = torch.exp(log_weights - log_weights.max())
    if weights is None:
        return a
    w = torch.as_tensor(weights, dtype=torch.float64, device=a.device)
    if w.shape != a.shape:
        raise ValueError(f"weights must have shape {tuple(a.shape)}, one per frame")
    return w * a


@dc.dataclass(frozen=True)
class MbarResult:
    """``f`` (K,) reduced free energies of the windows with f[0] = 0 and ``log_weights`` (N,) = -L_n, float64 on the device;
    ``iterations`` taken and the last ``delta`` = max |f' - f|.  ``theta`` (K, K) float64 on the device, the asymptotic
    covariance of the f_k (``uncertainties=True``; None otherwise)."""

    f: torch.Tensor
    log_weights: torch.Tensor
    iterations: int
    delta: float
    theta: torch.Tensor | None = None

    def f_error(self) -> torch.Tensor:
        """(K, K) float64: the standard deviation of f_i - f_j, sqrt(Theta_ii + Theta_jj - 2 Theta_ij), at uniform weights
        and for independent frames (module docstring)."""
        if self.theta is None:
            raise ValueError("MbarResult.f_error: solved without uncertainties=True, there is no covariance")
        d = torch.diagonal(self.theta)
        return torch.sqrt(torch.clamp(d[:, None] + d[None, :] - 2.0 * self.theta, min=0.0))

    def expect(self, values, weights=None) -> torch.Tensor:
        """<O> = sum_n w_n e^{lw_n} O_n / sum_n w_n e^{lw_n} for ``values`` (N,) or (N, ...) of the pooled frames;
        ``weights`` (N,) DiffTRe weights or None for uniform.  Differentiable in ``weights`` (and ``values``)."""
        a = _combined(self.log_weights, weights)
        v = torch.as_tensor(values, device=a.device).to(torch.float64)
        if v.shape[0] != a.shape[0]:
            raise ValueError(f"values must hold {a.shape[0]} frames along their first axis")
        a = a / a.sum()
        return (a.reshape(-1, *([1] * (v.dim() - 1))) * v).sum(0)

    def n_eff(self, weights=None) -> torch.Tensor:
        """Kish's effective sample size (sum a)^2 / sum a^2 of the combined weights a_n = w_n e^{lw_n}."""
        a = _combined(self.log_weights, weights)
        return a.sum() ** 2 / (a * a).sum()


def _theta(gram: np.ndarray, n: np.ndarray) -> np.ndarray:
    """The asymptotic covariance Theta = W^T (I - W N W^T)^+ W (Shirts and Chodera 2008, eq. 8 and D) of the log
    normalisation constants of the columns of W, from their Gram matrix G = W^T W alone: (A, A) float64 on the host.  ``n`` (A,)
    the columns' frame counts - 0 for a column that is not a sampled state (a bin, an observable).  Every column sums to 1
    (a sampled state at the solved f, an augmented column by its normalisation).
    With G = V diag(S^2) V^T:  Theta = V S M^+ S V^T,  M = I - S V^T N V S.  G may be singular (replica copies of one window
    are identical columns): a zero of S only drops out.  M has exactly one null vector, y = S V^T n (because G n = 1), so
    M^+ = (M + yy^T / |y|^2)^-1 - yy^T / |y|^2 with no threshold to guess; that direction adds a constant to Theta, which
    leaves every difference Theta_ii + Theta_jj - 2 Theta_ij alone."""
    gram, n = np.asarray(gram, dtype=np.float64), np.asarray(n, dtype=np.float64)
    lam, V = np.linalg.eigh(0.5 * (gram + gram.T))
    S = np.sqrt(np.clip(lam, 0.0, None))
    VS = V * S[None, :]
    M = np.eye(len(S)) - VS.T @ (n[:, None] * VS)
    y = VS.T @ n
    y /= np.linalg.norm(y)
    yy = np.outer(y, y)
    Mp = np.linalg.inv(M + yy) - yy
    theta = VS @ Mp @ VS.T
    if not np.isfinite(theta).all():
        raise FloatingPointError("mbar: non-finite covariance: a Gram matrix that is not at the solved f?")
    return 0.5 * (theta + theta.T)


def _sigma(theta: np.ndarray, i, j) -> np.ndarray:
    """The standard deviation of the difference of the log normalisation constants of columns i and j."""
    return np.sqrt(np.clip(theta[i, i] + theta[j, j] - 2.0 * theta[i, j], 0.0, None))


def _plan_theta(plan, f: torch.Tensor) -> torch.Tensor:
    g, _ = plan.gram(f, colsum=False)
    return torch.as_tensor(_theta(g.cpu().numpy(), plan._n_k), device=f.device)


def _counts(n_k) -> np.ndarray:
    n_k = np.ascontiguousarray(np.atleast_1d(n_k), dtype=np.int64)
    if n_k.ndim != 1:
        raise ValueError("n_k must hold one frame count per window")
    return n_k


def mbar(u_kn, n_k, tol: float = 1e-10, max_iter: int = 100_000, check_every: int = 32, solver: str = "fixed-point",
         uncertainties: bool = False) -> MbarResult:
    """MBAR of a reduced-energy matrix ``u_kn`` (K, N) float64 on the GPU - u_kn[k, n] is frame n evaluated in state k - whose
    frames were drawn N_k = ``n_k[k]`` from state k (sum = N; the order of the frames does not matter).  ``solver``
    "fixed-point" or "newton"; ``uncertainties`` fills ``MbarResult.theta`` (independent frames, uniform weights)."""
    u = torch.as_tensor(u_kn)
    if u.dim() != 2 or u.dtype != torch.float64:
        raise ValueError("u_kn must be a (K, N) float64 tensor")
    u = u.detach().contiguous()
    K, N = int(u.shape[0]), int(u.shape[1])
    n_k = _counts(n_k)
    if n_k.shape[0] != K:
        raise ValueError(f"n_k holds {n_k.shape[0]} counts, u_kn has {K} states")
    check(n_k, n_frames=N)
    if not bool(torch.isfinite(u).all()):
        raise ValueError("mbar: non-finite u_kn")
    plan = _MbarPlan(N, K, u.device)
    try:
        plan.set_matrix(u, n_k)
        f, it, d = plan.solve(tol, max_iter, check_every, solver=solver)
        return MbarResult(f=f, log_weights=plan.log_weights(f), iterations=it, delta=d, theta=_plan_theta(plan, f) if uncertainties else None)
    finally:
        plan.close()


def pooled(xi, n_k=None):
    """``xi`` (rows, R, P) as a simulator's ``state["pull"]`` -> ((N, P) window-major, n = r * rows + row - the order of
    ``SimulatorTrajectory.concat(out.observables)`` -, N_k = rows); an (N, P) tensor with its ``n_k`` passes through."""
    x = torch.as_tensor(xi)
    if x.dtype != torch.float64:
        raise ValueError("xi must be float64")
    if x.dim() == 3:
        if n_k is not None:
            raise ValueError("xi of shape (rows, R, P) carries its own counts: n_k must be None")
        rows, r, p = (int(s) for s in x.shape)
        return x.detach().permute(1, 0, 2).reshape(r * rows, p).contiguous(), np.full(r, rows, dtype=np.int64)
    if x.dim() != 2 or n_k is None:
        raise ValueError("xi must have shape (rows, R, P), or (N, P) with n_k")
    return x.detach().contiguous(), _counts(n_k)


def _umbrella_plan(xi, restraints, kT, n_k, topology):
    x, n_k = pooled(xi, n_k)
    K = int(n_k.shape[0])
    table = window_table(restraints, K, topology)
    if x.shape[1] != table.shape[1]:
        raise ValueError(f"xi holds {x.shape[1]} coordinates, the restraint set {table.shape[1]}")
    kTs = np.ascontiguousarray(np.broadcast_to(np.asarray(kT, dtype=np.float64), (K,)) if np.ndim(kT) == 0 else np.asarray(kT, dtype=np.float64))
    check(n_k, table=table, kT=kTs, xi=x.cpu().numpy())  # (one copy of xi to the host per fit: the non-finite check)
    plan = _MbarPlan(int(x.shape[0]), K, x.device)
    try:
        plan.set_windows(table, kTs, n_k, x)
    except Exception:
        plan.close()
        raise
    return plan, x


def mbar_umbrella(xi, restraints, kT, n_k=None, tol: float = 1e-10, max_iter: int = 100_000, check_every: int = 32,
                  topology=None, solver: str = "fixed-point", uncertainties: bool = False) -> MbarResult:
    """MBAR of umbrella windows: ``xi`` (rows, R, P) - ``out.state["pull"]``, R windows - or (N, P) with ``n_k``; window k is
    replica k of ``restraints`` (every pull coordinate contributes to the bias); ``kT`` in kJ/mol, one for all windows.  The
    K x N bias matrix is never stored.  ``topology`` only where a pull group is given by a selection.  ``solver`` and
    ``uncertainties`` as for ``mbar``."""
    plan, _ = _umbrella_plan(xi, restraints, kT, n_k, topology)
    try:
        f, it, d = plan.solve(tol, max_iter, check_every, solver=solver)
        return MbarResult(f=f, log_weights=plan.log_weights(f), iterations=it, delta=d, theta=_plan_theta(plan, f) if uncertainties else None)
    finally:
        plan.close()


class _PmfOp(torch.autograd.Function):
    """F_b of every bin as a function of the frame weights; backward is the analytic
    dF_b/dw_n = -kT e^{lw_n} ([n in b] / S_b - 1 / S), contracted with the incoming gradient over the occupied bins."""

    @staticmethod
    def forward(ctx, weights, pmf):
        sums = pmf._plan.binned_sum(pmf._seg, pmf._order, pmf.result.log_weights, weights.detach().contiguous(), pmf._shift)
        ctx.pmf, ctx.sums = pmf, sums
        return -pmf.kT * (torch.log(sums[:-1]) - torch.log(sums[-1]))

    @staticmethod
    def backward(ctx, g_out):
        pmf, sums = ctx.pmf, ctx.sums
        s_b, s = sums[:-1], sums[-1]
        occupied = s_b > 0.0
        g = torch.where(occupied, g_out.to(torch.float64), torch.zeros_like(s_b))
        per_bin = torch.cat([torch.where(occupied, g / s_b, torch.zeros_like(s_b)), torch.zeros(1, dtype=torch.float64, device=s_b.device)])
        return -pmf.kT * pmf._e * (per_bin[pmf._bin] - g.sum() / s), None


class UmbrellaPMF:
    """The free-energy profile of one pull coordinate from umbrella windows (module docstring).  ``fit(xi)`` once per stored
    trajectory, then ``pmf(weights)`` -> (B,) float64 kJ/mol on the GPU, differentiable in ``weights``; frames outside the
    edges count in the normalisation only.  ``uncertainty()`` and ``expect_error(values)`` are the asymptotic error bars of the
    unweighted profile and of ``result.expect(values)``: at the reference parameters (``weights=None``) and for independent
    frames - correlated frames make them too small by the square root of the statistical inefficiency."""

    def __init__(self, *, restraints, coordinate: int = 0, kT: float, edges, jacobian: str | None = None, topology=None,
                 tol: float = 1e-10, max_iter: int = 100_000, check_every: int = 32, solver: str = "fixed-point"):
        if solver not in SOLVERS:
            raise ValueError(f"solver {solver!r}: expected one of {SOLVERS}")
        self.solver = solver
        self.restraints, self.coordinate, self.kT, self.topology = restraints, int(coordinate), float(kT), topology
        self.tol, self.max_iter, self.check_every = tol, max_iter, check_every
        self.edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        if not 0 <= self.coordinate < len(restraints.pulls):
            raise ValueError(f"coordinate {coordinate} out of range [0, {len(restraints.pulls)})")
        if not (self.kT > 0.0 and math.isfinite(self.kT)):
            raise ValueError(f"kT {kT!r}: expected a positive energy")
        check([1], edges=self.edges)
        if jacobian not in (None, "distance"):
            raise ValueError(f"jacobian {jacobian!r}: expected None or 'distance'")
        self.jacobian = jacobian
        self._jac = None
        if jacobian == "distance":
            c = restraints.pulls[self.coordinate]
            if c.geometry != "distance" or not (self.centres > 0.0).all():
                raise ValueError("jacobian='distance' needs a coordinate of geometry 'distance' and bins at xi > 0")
            self._jac = self.kT * (sum(bool(a) for a in c.dim) - 1) * np.log(self.centres)
        self._plan = None
        self.result = self._gram = None

    @property
    def centres(self) -> np.ndarray:
        """(B,) bin centres."""
        return 0.5 * (self.edges[1:] + self.edges[:-1])

    def release(self) -> None:
        if self._plan is not None:
            self._plan.close()
        self._plan = None

    def fit(self, xi, n_k=None) -> MbarResult:
        """Solves MBAR for the frames ``xi`` (as ``mbar_umbrella``) and sorts them by bin, on the device."""
        self.release()
        plan, x = _umbrella_plan(xi, self.restraints, self.kT, n_k, self.topology)
        try:
            f, it, d = plan.solve(self.tol, self.max_iter, self.check_every, solver=self.solver)
            self.result = MbarResult(f=f, log_weights=plan.log_weights(f), iterations=it, delta=d)
        except Exception:
            plan.close()
            raise
        self._plan, self._gram = plan, None
        B = int(self.edges.shape[0]) - 1
        edges = torch.as_tensor(self.edges, device=x.device)
        b = torch.bucketize(x[:, self.coordinate].contiguous(), edges, right=True) - 1  # [e_b, e_b+1) -> b
        self._bin = torch.where((b < 0) | (b >= B), torch.full_like(b, B), b)            # outside: behind the last bin
        self._order = torch.sort(self._bin, stable=True).indices.contiguous()
        counts = torch.bincount(self._bin, minlength=B + 1)
        self._seg = torch.cat([torch.zeros(1, dtype=torch.int64, device=x.device), torch.cumsum(counts, 0)[:B]]).contiguous()
        self._shift = float(self.result.log_weights.max().item())
        self._e = torch.exp(self.result.log_weights - self._shift)
        return self.result

    def __call__(self, weights=None) -> torch.Tensor:
        if self._plan is None:
            raise _lib.MythosHipError("UmbrellaPMF: call fit(xi) first")
        lw = self.result.log_weights
        if weights is None:
            sums = self._plan.binned_sum(self._seg, self._order, lw, None, self._shift)
            F = -self.kT * (torch.log(sums[:-1]) - torch.log(sums[-1]))
        else:
            w = torch.as_tensor(weights, device=lw.device)
            if w.shape != lw.shape or w.dtype != torch.float64:
                raise ValueError(f"weights must be float64 of shape {tuple(lw.shape)}, one per frame")
            F = _PmfOp.apply(w, self)
        return F if self._jac is None else F + torch.as_tensor(self._jac, device=F.device)

    def _fitted(self, who: str):
        if self._plan is None:
            raise _lib.MythosHipError(f"UmbrellaPMF.{who}: call fit(xi) first")
        return self._plan, self.result.f

    def _augmented_theta(self, cross: np.ndarray, square: np.ndarray) -> np.ndarray:
        """Theta of the K windows followed by A columns x of count 0: ``cross`` (A, K) = sum_n x_n W_nk, ``square`` (A, A) =
        sum_n x_n x'_n."""
        plan, f = self._fitted("uncertainty")
        if self._gram is None:
            self._gram = plan.gram(f, colsum=False)[0].cpu().numpy()
        K, A = plan.K, cross.shape[0]
        g = np.zeros((K + A, K + A))
        g[:K, :K], g[K:, :K], g[:K, K:], g[K:, K:] = self._gram, cross, cross.T, square
        return _theta(g, np.concatenate([plan._n_k.astype(np.float64), np.zeros(A)]))

    def uncertainty(self, reference="min") -> torch.Tensor:
        """(B,) float64 kJ/mol on the GPU: the standard deviation of F_b - F_ref of the unweighted profile ``pmf()``; 0 at the
        reference bin - "min": the occupied bin of lowest F, or a bin index - and NaN at an empty bin.  The Jacobian term is a
        constant and does not enter.  Each occupied bin is one more column x_n = e^{lw_n} / S_b on the bin's frames next to the
        windows' in the estimator's asymptotic covariance."""
        plan, f = self._fitted("uncertainty")
        lw, B = self.result.log_weights, int(self.edges.shape[0]) - 1
        s1 = plan.binned_sum(self._seg, self._order, lw, None, self._shift)[:B].cpu().numpy()     # sum e over the bin
        s2 = plan.binned_sum(self._seg, self._order, lw, self._e, self._shift)[:B].cpu().numpy()  # sum e^2
        occ = np.flatnonzero(s1 > 0.0)
        if reference == "min":
            if not len(occ):
                raise ValueError("UmbrellaPMF.uncertainty: every bin is empty")
            ref = int(occ[np.argmax(s1[occ])])
        elif isinstance(reference, (int, np.integer)) and not isinstance(reference, bool) and 0 <= int(reference) < B:
            ref = int(reference)
            if not s1[ref] > 0.0:
                raise ValueError(f"UmbrellaPMF.uncertainty: the reference bin {ref} is empty")
        else:
            raise ValueError(f"reference {reference!r}: expected 'min' or a bin index in [0, {B})")
        cross = plan.segment_moments(f, self._seg, self._order, self._e).cpu().numpy()[occ] / s1[occ, None]
        theta = self._augmented_theta(cross, np.diag(s2[occ] / s1[occ] ** 2))
        at = plan.K + np.arange(len(occ))
        out = np.full(B, np.nan)
        out[occ] = self.kT * _sigma(theta, at, plan.K + int(np.searchsorted(occ, ref)))
        out[ref] = 0.0
        return torch.as_tensor(out, device=lw.device)

    def expect_error(self, values) -> torch.Tensor:
        """The standard deviation of ``result.expect(values)`` for ``values`` (N,) or (N, E): () or (E,) float64 on the GPU.  Two
        columns per observable, e^{lw} A' / sum e^{lw} A' with A' = A - min A + 1 > 0 and e^{lw} / sum e^{lw}:
        sigma^2 = <A'>^2 (Theta_AA + Theta_aa - 2 Theta_Aa)."""
        plan, f = self._fitted("expect_error")
        v = torch.as_tensor(values, device=f.device).to(torch.float64)
        if v.dim() not in (1, 2) or v.shape[0] != plan.N:
            raise ValueError(f"values must have shape ({plan.N},) or ({plan.N}, E)")
        if not bool(torch.isfinite(v).all()):
            raise ValueError("UmbrellaPMF.expect_error: non-finite values")
        cols = v.reshape(plan.N, -1)
        a = (self._e / self._e.sum()).contiguous()
        cross_a = plan.segment_moments(f, v=a)[0].cpu().numpy()
        out = np.zeros(cols.shape[1])
        for e in range(cols.shape[1]):
            shifted = cols[:, e] - cols[:, e].min() + 1.0
            mean = float((a * shifted).sum().item())
            x = (a * shifted / mean).contiguous()
            cross = np.stack([plan.segment_moments(f, v=x)[0].cpu().numpy(), cross_a])
            xa = float((x * a).sum().item())
            theta = self._augmented_theta(cross, np.array([[float((x * x).sum().item()), xa], [xa, float((a * a).sum().item())]]))
            out[e] = mean * _sigma(theta, plan.K, plan.K + 1)
        return torch.as_tensor(out.reshape(tuple(v.shape[1:])), device=f.device)
