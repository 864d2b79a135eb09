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

Correlated frames: ``statistical_inefficiency(xi)`` is g = 1 + 2 tau of every window's time series (autocorrelation
functions from csrc/timeseries.hip), and ``bootstrap=B`` (``mbar``, ``mbar_umbrella``, ``UmbrellaPMF.fit``; ``solver="newton"``)
solves B moving-block bootstrap replicates next to the estimate.  ``block_resample`` redraws every window as blocks of
consecutive frames - ``block="auto"``: l_k = min(N_k, ceil(3 max_p g_kp)) - and a replicate is the integer multiplicity m_bn of
every frame, never a gathered copy of the frames.  Replicate b solves sum_n m_bn W_bnk = 1.  About the solved f^, with
delta_b = f_b - f^ and t^_jn = N_j W^_nj,

    D_bn = sum_j t^_jn e^{delta_bj},        W_bnk = W^_nk e^{delta_bk} / D_bn,        e^{lw_bn} = e^{-L^_n} / D_bn

so the exponentials of a frame are formed once and shared by the replicates (``mythos_mbar_boot_colsums``,
``mythos_mbar_boot_binned``).  ``_MbarPlan._bootstrap`` is a chord iteration with the Hessian H^ at f^, inverted once: per
iteration, for all replicates of a batch, the chord candidate delta_b - H^-1 g_b (g_bk = N_k (s_bk - 1) / N) and the
self-consistent candidate delta_b - ln s_b, both with delta_b0 = 0, are evaluated in one launch of 2 B rows and the one with
the smaller |g| is kept, until max_k |ln s_bk - ln s_b0| <= ``tol`` for every replicate (``MbarNotConverged`` after 100
iterations, naming how many replicates are left).  ``MbarResult.f_error("bootstrap")``, ``UmbrellaPMF.uncertainty(method=
"bootstrap", weights=w)``, ``interval`` and ``expect_error(values, method="bootstrap", weights=w)`` are statistics over the
replicates; with DiffTRe ``weights`` the replicates' binned sums are re-formed in one launch per batch.
``subsample_correlated`` instead thins the frames to one per g, the input of the asymptotic error bars.

Not built: circular and stationary bootstraps, a per-replicate Hessian refresh, bootstrap for more windows than fit the
kernel's LDS (about 100 of one coordinate); states with N_k = 0, moving windows (``rate``), 2-D profiles.
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

    def _boot_args(self, f, delta, mult) -> int:
        self._ours(f, (self.K,), "f_hat")
        if not (isinstance(delta, torch.Tensor) and delta.dim() == 2):
            raise ValueError("delta must be a (B, K) tensor")
        n_boot = int(delta.shape[0])
        self._ours(delta, (n_boot, self.K), "delta")
        if not (isinstance(mult, torch.Tensor) and mult.dtype == torch.uint16 and mult.device == self.device
                and tuple(mult.shape) == (n_boot, self.N) and mult.is_contiguous()):
            raise ValueError(f"mult must be a contiguous uint16 tensor of shape ({n_boot}, {self.N}) on {self.device}")
        return n_boot

    def boot_colsums(self, f: torch.Tensor, delta: torch.Tensor, mult: torch.Tensor) -> torch.Tensor:
        """(B, K): s_bk = sum_n mult[b, n] W_bnk of replicates ``delta`` (B, K) away from ``f`` (module docstring)."""
        n_boot = self._boot_args(f, delta, mult)
        out = torch.empty(n_boot, self.K, dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mythos_mbar_boot_colsums(self._h, _lib.ptr(f), n_boot, _lib.ptr(delta), _lib.ptr(mult), _lib.ptr(out),
                                                      _lib.stream(self.device)), "mbar_boot_colsums")
        return out

    def boot_binned(self, f: torch.Tensor, delta: torch.Tensor, mult: torch.Tensor, seg_start=None, order=None, v=None,
                    shift: float = 0.0) -> torch.Tensor:
        """(B, n_seg, max(E, 1)): per replicate and segment the sum of mult[b, n] v[n, e] exp(-L_n - shift) / D_bn; ``order``
        and ``seg_start`` as for ``segment_moments``, ``v`` (N, E) with E <= 8 or None for 1."""
        n_boot = self._boot_args(f, delta, mult)
        n_cols = 0
        if v is not None:
            if not (isinstance(v, torch.Tensor) and v.dim() == 2):
                raise ValueError("v must be an (N, E) tensor")
            n_cols = int(v.shape[1])
            self._ours(v, (self.N, n_cols), "v")
        if (order is None) != (seg_start is None):
            raise ValueError("order and seg_start come together")
        n_seg = 1
        if order is not None:
            n_seg = int(seg_start.shape[0]) - 1
            if (order.dtype != torch.int64 or tuple(order.shape) != (self.N,) or seg_start.dtype != torch.int64 or seg_start.dim() != 1
                    or order.device != self.device or seg_start.device != self.device or not (order.is_contiguous() and seg_start.is_contiguous())):
                raise ValueError("order must be int64 of shape (N,), seg_start int64 of shape (n_seg + 1,), contiguous on the plan's device")
        out = torch.empty(n_boot, max(n_seg, 0), max(n_cols, 1), dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mythos_mbar_boot_binned(self._h, _lib.ptr(f), n_boot, _lib.ptr(delta), _lib.ptr(mult), n_seg, _lib.ptr(seg_start),
                                                     _lib.ptr(order), n_cols, _lib.ptr(v if n_cols else None), float(shift), _lib.ptr(out),
                                                     _lib.stream(self.device)), "mbar_boot_binned")
        return out

    def _bootstrap(self, f: torch.Tensor, batches, tol: float, max_iter: int = 100) -> torch.Tensor:
        """The replicates' delta_b = f_b - f (B, K) on the device, delta_b0 = 0: a chord iteration with the Hessian at the solved
        ``f``, all replicates of a batch at once (module docstring).  ``batches`` yields (B_c, N) uint16 multiplicities.  Raises
        ``MbarNotConverged`` if any replicate is left above ``tol`` after ``max_iter`` iterations."""
        tol, max_iter = float(tol), int(max_iter)
        if not tol > 0.0 or max_iter < 1:
            raise ValueError("tol > 0 and max_iter >= 1 required")
        n = self._n_k.astype(np.float64)
        total, K = n.sum(), self.K
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=self.device)  # noqa: E731
        h_inv = None
        if K > 1:
            g_d, s_d = self.gram(f)
            G, s = g_d.cpu().numpy(), s_d.cpu().numpy()
            hess = (np.diag(n * s) - (n[:, None] * n[None, :]) * G) / total
            try:
                h_inv = np.linalg.inv(hess[1:, 1:])
            except np.linalg.LinAlgError:
                h_inv = None  # (the self-consistent candidate alone)
        out = []
        for m in batches:
            B = int(m.shape[0])
            both = torch.cat([m.view(torch.int16), m.view(torch.int16)]).contiguous().view(torch.uint16)
            delta = np.zeros((B, K))
            s = self.boot_colsums(f, dev(delta), m).cpu().numpy()
            for it in range(0, max_iter + 1):
                if not (np.isfinite(s).all() and (s > 0.0).all()):
                    raise FloatingPointError(f"mbar: non-finite or empty column sums in bootstrap iteration {it}: a replicate without overlap?")
                ln_s = np.log(s)
                d = np.abs(ln_s - ln_s[:, :1]).max(axis=1)  # max |f' - f| of one fixed-point map, per replicate
                if (d <= tol).all():
                    break
                if it == max_iter:
                    raise MbarNotConverged(f"mbar: bootstrap not converged within max_iter = {max_iter}: {int((d > tol).sum())} of {B} "
                                           f"replicates above tol = {tol:.3e}, the worst delta = max |f' - f| is {d.max():.3e}", float(d.max()), max_iter)
                grad = n[None, :] * (s - 1.0) / total
                fixed = delta - ln_s + ln_s[:, :1]
                chord = fixed
                if h_inv is not None:
                    chord = delta.copy()
                    chord[:, 1:] -= grad[:, 1:] @ h_inv.T
                    chord = np.where(np.isfinite(chord).all(axis=1, keepdims=True), chord, fixed)
                cands = np.concatenate([chord, fixed])
                s2 = self.boot_colsums(f, dev(cands), both).cpu().numpy()
                with np.errstate(invalid="ignore"):
                    norm = np.linalg.norm(n[None, :] * (s2 - 1.0) / total, axis=1)
                norm = np.where(np.isfinite(s2).all(axis=1) & (s2 > 0.0).all(axis=1), norm, np.inf)
                take = np.where(norm[B:] < norm[:B], B, 0) + np.arange(B)  # the chord candidate unless the other is better
                if not np.isfinite(norm[take]).all():
                    raise FloatingPointError(f"mbar: no finite candidate in bootstrap iteration {it + 1}: a replicate without overlap?")
                delta, s = cands[take], s2[take]
            out.append(dev(delta))
        return torch.cat(out) if out else torch.zeros(0, K, dtype=torch.float64, device=self.device)

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
    boot_f: torch.Tensor | None = None  # (B, K) the block-bootstrap replicates' f, float64 on the device (``bootstrap=B``)
    g: np.ndarray | None = None         # (K,) the windows' statistical inefficiencies (block="auto"; None otherwise)
    block: np.ndarray | None = None     # (K,) the block lengths of the resampling

    def f_error(self, method: str = "asymptotic") -> torch.Tensor:
        """(K, K) float64: the standard deviation of f_i - f_j.  "asymptotic": sqrt(Theta_ii + Theta_jj - 2 Theta_ij), at uniform
        weights and for independent frames (module docstring).  "bootstrap": the sample standard deviation (ddof = 1) over the
        block-bootstrap replicates ``boot_f``, which holds for correlated frames."""
        if method == "bootstrap":
            if self.boot_f is None or self.boot_f.shape[0] < 2:
                raise ValueError("MbarResult.f_error: solved without bootstrap >= 2, there are no replicates")
            return torch.std(self.boot_f[:, :, None] - self.boot_f[:, None, :], dim=0, unbiased=True)
        if method != "asymptotic":
            raise ValueError(f"method {method!r}: expected one of {ERROR_METHODS}")
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
         uncertainties: bool = False, bootstrap: int = 0, block="auto", boot_seed: int = 0) -> MbarResult:
    """MBAR of a reduced-energy matrix ``u_kn`` (K, N) float64 on the GPU - u_kn[k, n] is frame n evaluated in state k - whose
    frames were drawn N_k = ``n_k[k]`` from state k (sum = N; the order of the frames does not matter).  ``solver``
    "fixed-point" or "newton"; ``uncertainties`` fills ``MbarResult.theta`` (independent frames, uniform weights).
    ``bootstrap=B`` > 0 (``solver="newton"`` only) adds B moving-block bootstrap replicates, ``MbarResult.boot_f``: for it the
    frames of a state must be CONTIGUOUS (state 0's N_0 frames first) and TIME-ORDERED inside the state.  ``block`` is the
    block length, an int or one per state, or "auto": from the statistical inefficiency of each state's own reduced energy
    u_kn[k, n] over its frames; ``boot_seed`` seeds the resampling."""
    u = torch.as_tensor(u_kn)
    if u.dim() != 2 or u.dtype != torch.float64:
        raise ValueError("u_kn must be a (K, N) float64 tensor")
    u = u.detach().contiguous()
    K, N = int(u.shape[0]), int(u.shape[1])
    n_k = _counts(n_k)
    if n_k.shape[0] != K:
        raise ValueError(f"n_k holds {n_k.shape[0]} counts, u_kn has {K} states")
    bootstrap = _check_bootstrap(bootstrap, solver)
    check(n_k, n_frames=N)
    if not bool(torch.isfinite(u).all()):
        raise ValueError("mbar: non-finite u_kn")
    plan = _MbarPlan(N, K, u.device)
    try:
        plan.set_matrix(u, n_k)
        f, it, d = plan.solve(tol, max_iter, check_every, solver=solver)
        extra = {}
        if bootstrap:
            own = torch.as_tensor(np.repeat(np.arange(K), n_k), device=u.device)
            series = u[own, torch.arange(N, device=u.device)][:, None].contiguous() if isinstance(block, str) else None
            extra = _boot_fields(plan, f, series, n_k, bootstrap, block, boot_seed, tol)[0]
        return MbarResult(f=f, log_weights=plan.log_weights(f), iterations=it, delta=d, theta=_plan_theta(plan, f) if uncertainties else None,
                          **extra)
    finally:
        plan.close()


def _boot_fields(plan, f, series, n_k, bootstrap, block, boot_seed, tol) -> tuple:
    """(the bootstrap's fields of an ``MbarResult``, the ``BlockResample``, delta (B, K)): the last two for ``UmbrellaPMF``."""
    resample, g = _resample_for(plan, series, n_k, bootstrap, block, boot_seed)
    delta = plan._bootstrap(f, resample.batches(plan.device), tol, BOOT_MAX_ITER)
    return dict(boot_f=f[None, :] + delta, g=g, block=resample.block), resample, delta


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


def _offsets(n_k: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum(n_k)]), dtype=np.int64)


def check_series(n_k, x=None, n_rows=None, n_cols=None) -> None:
    """What the time-series entry points refuse, without a device (mythos_timeseries_check): raises ValueError with its
    message.  ``x`` (N, E) on the host, or None with ``n_rows`` and ``n_cols``."""
    n_k = _counts(n_k)
    x = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    if x is not None and x.ndim != 2:
        raise ValueError("the series must have shape (N, E)")
    N = int(x.shape[0]) if x is not None else int(n_k.sum() if n_rows is None else n_rows)
    E = int(x.shape[1]) if x is not None else int(1 if n_cols is None else n_cols)
    off = _offsets(n_k)
    _lib.check(_lib.load().mythos_timeseries_check(N, E, int(n_k.shape[0]), off.ctypes.data_as(_I64P),
                                                   None if x is None or x.size == 0 else x.ctypes.data_as(_lib.c_double_p)), "timeseries_check")


def statistical_inefficiency(series, n_k=None, mintime: int = 3, lag_block: int = 256) -> torch.Tensor:
    """(K, E) float64 on the GPU: the statistical inefficiency g = 1 + 2 tau of every window's time series, so that N_k / g
    frames of the N_k count as independent.  ``series`` is (rows, R, P) as ``out.state["pull"]``, or (N, E) with ``n_k``:
    window-major, time-ordered inside a window, as ``pooled`` delivers the frames.  With mu and v the mean and variance of a
    series of length T,

        C(t) = sum_{i < T - t} (x_i - mu)(x_{i+t} - mu) / ((T - t) v),      g = max(1, 1 + 2 sum_{t=1}^{t* - 1} C(t) (1 - t / T))

    and t* the first t > ``mintime`` with C(t) <= 0 (T - 1 if there is none); g = 1 for T <= 2 or v = 0 (pymbar's
    ``statistical_inefficiency``).  C comes from ``mythos_timeseries_autocorr`` in blocks of ``lag_block`` lags of all series
    at once until every series has crossed zero - one word read back per block -, g is formed on the device."""
    x, n_k = pooled(series, n_k)
    mintime, lag_block = int(mintime), int(lag_block)
    if mintime < 0 or not 1 <= lag_block <= 1 << 16:
        raise ValueError("mintime >= 0 and 1 <= lag_block <= 65536 required")
    if x.device.type != "cuda":
        raise _lib.MythosHipError("the autocorrelation functions are computed by the HIP library: the series must live on a GPU "
                                  "(mythos_amd has no CPU fallback)")
    check_series(n_k, x=x.cpu().numpy())  # (one copy to the host per call: the non-finite check)
    lib, dev = _lib.load(), x.device
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    N, E, K = int(x.shape[0]), int(x.shape[1]), int(n_k.shape[0])
    off = _offsets(n_k)
    off_d = torch.as_tensor(off, device=dev)
    mean, var = (torch.empty(K, E, dtype=torch.float64, device=dev) for _ in range(2))
    head = (_lib.ptr(x), N, E, K, off.ctypes.data_as(_I64P), _lib.ptr(off_d))
    _lib.check(lib.mythos_timeseries_moments(*head, _lib.ptr(mean), _lib.ptr(var), index, _lib.stream(dev)), "timeseries_moments")
    T = torch.as_tensor(n_k, device=dev).repeat_interleave(E)[:, None]  # (K E, 1)
    t_max, t, blocks = int(n_k.max()), 1, []
    crossed = torch.zeros(K * E, dtype=torch.bool, device=dev)
    while t <= t_max - 2:  # the lags 1 ... T - 2 enter g
        n = min(lag_block, t_max - 1 - t)
        out = torch.empty(K * E, n, dtype=torch.float64, device=dev)
        _lib.check(lib.mythos_timeseries_autocorr(*head, _lib.ptr(mean), _lib.ptr(var), t, n, _lib.ptr(out), index, _lib.stream(dev)),
                   "timeseries_autocorr")
        tt = torch.arange(t, t + n, device=dev)[None, :]
        crossed |= ((out <= 0.0) & (tt > mintime) & (tt <= T - 2)).any(dim=1)
        blocks.append(out)
        t += n
        if bool((crossed | (t > T[:, 0] - 2)).all()):
            break
    g = torch.ones(K * E, dtype=torch.float64, device=dev)
    if blocks:
        c = torch.cat(blocks, dim=1)
        tt = torch.arange(1, 1 + c.shape[1], device=dev)[None, :]
        cross = (c <= 0.0) & (tt > mintime) & (tt <= T - 2)
        t_star = torch.where(cross, tt, T - 1).min(dim=1, keepdim=True).values
        terms = torch.where(tt < t_star, c * (1.0 - tt.to(torch.float64) / T.to(torch.float64)), torch.zeros_like(c))
        g = torch.clamp(1.0 + 2.0 * terms.sum(dim=1), min=1.0)
        g = torch.where((T[:, 0] <= 2) | (var.reshape(-1) <= 0.0), torch.ones_like(g), g)
    return g.reshape(K, E)


BOOT_BLOCK_FACTOR = 3            # c of block="auto": block length = ceil(c max_p g_kp), see DESIGN section 3.5o
BOOT_BATCH_BYTES = 1 << 27       # bound on the (B_c, N) uint16 multiplicities of one batch of replicates
BOOT_MAX_BLOCKS = 65_535         # blocks per window: a frame's multiplicity fits uint16
ERROR_METHODS = ("asymptotic", "bootstrap")


def auto_block(g, n_k) -> np.ndarray:
    """(K,) int64: l_k = min(N_k, ceil(BOOT_BLOCK_FACTOR max_p g_kp)) for ``g`` (K,) or (K, P)."""
    n_k = _counts(n_k)
    g = np.asarray(g.cpu().numpy() if isinstance(g, torch.Tensor) else g, dtype=np.float64).reshape(n_k.shape[0], -1).max(axis=1)
    if not (np.isfinite(g).all() and (g >= 1.0).all()):
        raise ValueError("auto_block: a statistical inefficiency below 1 or non-finite")
    return np.minimum(n_k, np.ceil(BOOT_BLOCK_FACTOR * g).astype(np.int64))


@dc.dataclass(frozen=True)
class BlockResample:
    """A moving-block bootstrap inside each window (``block_resample``).  ``block`` (K,) the block lengths l_k; ``starts`` one
    (n_boot, M_k) int64 array per window, M_k = ceil(N_k / l_k): the first frame, inside the window, of every block of every
    replicate; ``lengths`` one (M_k,) array per window: l_k, and N_k - (M_k - 1) l_k for the last block."""

    n_k: np.ndarray
    block: np.ndarray
    n_boot: int
    seed: int
    starts: tuple
    lengths: tuple

    def batch_size(self, max_bytes: int = BOOT_BATCH_BYTES) -> int:
        """Replicates per batch: as many as keep (B_c, N) uint16 at or below ``max_bytes`` (at least one)."""
        return max(1, min(self.n_boot, int(max_bytes) // (2 * int(self.n_k.sum()))))

    def multiplicities(self, lo: int, hi: int, device) -> torch.Tensor:
        """(hi - lo, N) uint16 on ``device``: how often replicate b = lo ... hi - 1 holds frame n.  Integer operations only - a
        difference array (+1 at a block's first frame, -1 behind its last) and a prefix sum along the frames -, so every
        window's multiplicities sum to N_k exactly."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.n_boot:
            raise ValueError(f"replicates [{lo}, {hi}) out of range [0, {self.n_boot})")
        N, rows = int(self.n_k.sum()), hi - lo
        off = _offsets(self.n_k)
        first = np.concatenate([(off[k] + s[lo:hi]) + np.arange(rows)[:, None] * (N + 1) for k, s in enumerate(self.starts)], axis=1)
        behind = first + np.concatenate(self.lengths)[None, :]
        diff = torch.zeros(rows * (N + 1), dtype=torch.int32, device=device)
        one = torch.ones(first.size, dtype=torch.int32, device=device)
        diff.index_add_(0, torch.as_tensor(first.reshape(-1), device=device), one)
        diff.index_add_(0, torch.as_tensor(behind.reshape(-1), device=device), -one)
        # (through int16, bit for bit: every dtype conversion and copy kernel knows that type)
        return torch.cumsum(diff.view(rows, N + 1)[:, :N], dim=1, dtype=torch.int32).to(torch.int16).contiguous().view(torch.uint16)

    def batches(self, device, max_bytes: int = BOOT_BATCH_BYTES):
        """Yields the (B_c, N) uint16 multiplicities batch by batch, replicates in order."""
        step = self.batch_size(max_bytes)
        for lo in range(0, self.n_boot, step):
            yield self.multiplicities(lo, min(lo + step, self.n_boot), device)


def block_resample(n_k, block, n_boot: int, seed: int = 0) -> BlockResample:
    """A moving-block bootstrap inside each window: window k of N_k time-ordered frames is redrawn as M_k = ceil(N_k / l_k)
    blocks of consecutive frames, every block l_k long except the last, N_k - (M_k - 1) l_k, and every block's first frame
    uniform on [0, N_k - length].  ``block`` is an int or a (K,) array of block lengths (``auto_block`` makes them from the
    statistical inefficiencies).  The starts come from ``numpy.random.default_rng(seed)`` in this order: window 0 first, and
    for a window one call ``rng.integers(0, N_k - lengths + 1, size=(n_boot, M_k))`` - replicate-major, block-minor."""
    n_k = _counts(n_k)
    K, n_boot = int(n_k.shape[0]), int(n_boot)
    if (n_k < 1).any():
        raise ValueError("block_resample: N_k < 1 (states without frames are not built)")
    if n_boot < 1:
        raise ValueError("block_resample: n_boot < 1 (at least one replicate)")
    raw = np.asarray(block)
    if raw.dtype.kind not in "iu" or raw.shape not in ((), (K,)):
        raise ValueError(f"block must be an int or {K} ints, one block length per window")
    block = np.ascontiguousarray(np.broadcast_to(raw, (K,)), dtype=np.int64)
    if (block < 1).any():
        raise ValueError(f"block_resample: a block shorter than 1 (window {int(np.argmax(block < 1))})")
    block = np.minimum(block, n_k)
    count = -(-n_k // block)
    if (count > BOOT_MAX_BLOCKS).any():
        k = int(np.argmax(count > BOOT_MAX_BLOCKS))
        raise ValueError(f"block_resample: window {k} has more than {BOOT_MAX_BLOCKS} blocks ({int(count[k])}): the multiplicities are uint16")
    rng = np.random.default_rng(seed)
    starts, lengths = [], []
    for k in range(K):
        length = np.full(int(count[k]), block[k], dtype=np.int64)
        length[-1] = n_k[k] - (count[k] - 1) * block[k]
        starts.append(rng.integers(0, n_k[k] - length + 1, size=(n_boot, int(count[k])), dtype=np.int64))
        lengths.append(length)
    return BlockResample(n_k=n_k, block=block, n_boot=n_boot, seed=int(seed), starts=tuple(starts), lengths=tuple(lengths))


def subsample_indices(n_k, g) -> tuple:
    """(the kept frames' pooled indices, n_k'): per window the frames at round-half-up(j g_k), j = 0, 1, ... while that is
    below N_k, duplicates dropped."""
    n_k = _counts(n_k)
    g = np.asarray(g.cpu().numpy() if isinstance(g, torch.Tensor) else g, dtype=np.float64).reshape(n_k.shape[0], -1).max(axis=1)
    if not (np.isfinite(g).all() and (g > 0.0).all()):
        raise ValueError("subsample_correlated: g must be positive and finite")
    off, keep, kept = _offsets(n_k), [], []
    for k in range(n_k.shape[0]):
        j = np.arange(int(math.ceil(n_k[k] / g[k])) + 1)
        idx = np.unique(np.floor(j * g[k] + 0.5).astype(np.int64))
        idx = idx[idx < n_k[k]]
        keep.append(off[k] + idx), kept.append(len(idx))
    return np.concatenate(keep), np.asarray(kept, dtype=np.int64)


def subsample_correlated(xi, g=None, n_k=None):
    """(xi' (N', P), n_k'): the frames ``subsample_indices`` keeps, the input of the asymptotic error bars when the caller
    wants decorrelated frames.  ``g`` (K,) or (K, P) - a window takes its largest -, or None for
    ``statistical_inefficiency(xi, n_k)``."""
    x, n_k = pooled(xi, n_k)
    if g is None:
        g = statistical_inefficiency(x, n_k)
    keep, kept = subsample_indices(n_k, g)
    return x[torch.as_tensor(keep, device=x.device)].contiguous(), kept


def _resample_for(plan, series, n_k, bootstrap, block, boot_seed):
    """(BlockResample, g (K,) or None) for the public entry points; ``series`` (N, E) on the device, for block="auto"."""
    g = None
    if isinstance(block, str):
        if block != "auto":
            raise ValueError(f"block {block!r}: expected 'auto', an int or one int per window")
        g = statistical_inefficiency(series, n_k).max(dim=1).values.cpu().numpy()
        block = auto_block(g, n_k)
    return block_resample(n_k, block, bootstrap, boot_seed), g


def _check_bootstrap(bootstrap, solver) -> int:
    bootstrap = int(bootstrap)
    if bootstrap < 0:
        raise ValueError("bootstrap >= 0 required")
    if bootstrap and solver != "newton":
        raise ValueError(f"bootstrap > 0 requires solver='newton' (the replicates start from its Hessian), not solver={solver!r}")
    return bootstrap


BOOT_MAX_ITER = 100  # chord iterations of the batched bootstrap solve


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
                  topology=None, solver: str = "fixed-point", uncertainties: bool = False, bootstrap: int = 0, block="auto",
                  boot_seed: int = 0) -> MbarResult:
    """MBAR of umbrella windows: ``xi`` (rows, R, P) - ``out.state["pull"]``, R windows - or (N, P) with ``n_k``; window k is
    replica k of ``restraints`` (every pull coordinate contributes to the bias); ``kT`` in kJ/mol, one for all windows.  The
    K x N bias matrix is never stored.  ``topology`` only where a pull group is given by a selection.  ``solver`` and
    ``uncertainties`` as for ``mbar``.  ``bootstrap=B`` > 0 (``solver="newton"`` only) adds B moving-block bootstrap replicates
    (``boot_f``, ``g``, ``block``; module docstring): the frames must be time-ordered inside a window, as ``pooled`` delivers
    them.  ``block`` "auto" (from the statistical inefficiency of xi), an int or one per window; ``boot_seed``."""
    bootstrap = _check_bootstrap(bootstrap, solver)
    plan, x = _umbrella_plan(xi, restraints, kT, n_k, topology)
    try:
        f, it, d = plan.solve(tol, max_iter, check_every, solver=solver)
        extra = _boot_fields(plan, f, x, plan._n_k, bootstrap, block, boot_seed, tol)[0] if bootstrap else {}
        return MbarResult(f=f, log_weights=plan.log_weights(f), iterations=it, delta=d, theta=_plan_theta(plan, f) if uncertainties else None,
                          **extra)
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
    frames - correlated frames make them too small by the square root of the statistical inefficiency.  After
    ``fit(xi, bootstrap=B)`` the same two with ``method="bootstrap"``, and ``interval``, are statistics over B moving-block
    bootstrap replicates: they hold for correlated frames and take DiffTRe ``weights``."""

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
        self.result = self._gram = self._resample = self._boot_delta = None

    @property
    def centres(self) -> np.ndarray:
        """(B,) bin centres."""
        return 0.5 * (self.edges[1:] + self.edges[:-1])

    def release(self) -> None:
        if self._plan is not None:
            self._plan.close()
        self._plan = None

    def fit(self, xi, n_k=None, bootstrap: int = 0, block="auto", boot_seed: int = 0) -> MbarResult:
        """Solves MBAR for the frames ``xi`` (as ``mbar_umbrella``) and sorts them by bin, on the device.  ``bootstrap=B`` > 0
        (``solver="newton"`` only) also solves B moving-block bootstrap replicates and keeps their delta_b = f_b - f on the plan:
        the input of ``uncertainty(method="bootstrap")``, ``interval`` and ``expect_error(method="bootstrap")``, which
        regenerate the multiplicities from ``boot_seed`` batch by batch."""
        self.release()
        bootstrap = _check_bootstrap(bootstrap, self.solver)
        plan, x = _umbrella_plan(xi, self.restraints, self.kT, n_k, self.topology)
        self._resample = self._boot_delta = None
        try:
            f, it, d = plan.solve(self.tol, self.max_iter, self.check_every, solver=self.solver)
            extra = {}
            if bootstrap:
                extra, self._resample, self._boot_delta = _boot_fields(plan, f, x, plan._n_k, bootstrap, block, boot_seed, self.tol)
            self.result = MbarResult(f=f, log_weights=plan.log_weights(f), iterations=it, delta=d, **extra)
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

    def _boot_weights(self, who: str, weights):
        plan, f = self._fitted(who)
        if self._boot_delta is None:
            raise ValueError(f"UmbrellaPMF.{who}: fitted without bootstrap=B, there are no replicates")
        if weights is None:
            return plan, f, None
        w = torch.as_tensor(weights, device=f.device)
        if tuple(w.shape) != (plan.N,) or w.dtype != torch.float64:
            raise ValueError(f"weights must be float64 of shape ({plan.N},), one per frame")
        return plan, f, w.detach().contiguous()

    def _boot_sums(self, who: str, v, binned: bool) -> np.ndarray:
        """(replicates, segments, E) on the host: ``boot_binned`` of every batch, multiplicities regenerated from the seed.
        ``binned``: the bins' segments and one more for the frames outside; otherwise one segment over all frames."""
        plan, f = self._fitted(who)
        out, lo = [], 0
        seg = torch.cat([self._seg, torch.full((1,), plan.N, dtype=torch.int64, device=f.device)]).contiguous() if binned else None
        for m in self._resample.batches(plan.device):
            delta = self._boot_delta[lo:lo + m.shape[0]].contiguous()
            out.append(plan.boot_binned(f, delta, m, seg, self._order if binned else None, v, self._shift).cpu().numpy())
            lo += m.shape[0]
        return np.concatenate(out)

    def boot_profiles(self, weights=None) -> torch.Tensor:
        """(replicates, B) float64 kJ/mol on the GPU: the profile of every bootstrap replicate, -kT [ln S_b,bin - ln S_b] plus
        the Jacobian term, under DiffTRe ``weights`` (N,) or uniform; +inf where a bin is empty in a replicate.  One launch per
        batch over all its replicates."""
        plan, f, w = self._boot_weights("boot_profiles", weights)
        sums = self._boot_sums("boot_profiles", None if w is None else w[:, None].contiguous(), True)[:, :, 0]
        with np.errstate(divide="ignore"):
            F = -self.kT * (np.log(sums[:, :-1]) - np.log(sums.sum(axis=1))[:, None])
        if self._jac is not None:
            F = F + self._jac[None, :]
        return torch.as_tensor(F, device=f.device)

    def interval(self, level: float = 0.95, weights=None) -> torch.Tensor:
        """(2, B) float64 kJ/mol on the GPU: the (1 - level) / 2 and (1 + level) / 2 percentiles (linear interpolation) of F_b
        over the bootstrap replicates in which the bin is occupied; NaN where that is fewer than two."""
        if not 0.0 < float(level) < 1.0:
            raise ValueError("0 < level < 1 required")
        F = self.boot_profiles(weights).cpu().numpy()
        out = np.full((2, F.shape[1]), np.nan)
        for b in range(F.shape[1]):
            col = F[np.isfinite(F[:, b]), b]
            if len(col) >= 2:
                out[:, b] = np.percentile(col, [50.0 * (1.0 - level), 50.0 * (1.0 + level)])
        return torch.as_tensor(out, device=self.result.f.device)

    def _boot_uncertainty(self, reference, weights) -> torch.Tensor:
        F = self.boot_profiles(weights).cpu().numpy()
        central = self(weights).detach().cpu().numpy()
        if self._jac is not None:  # (a constant per bin: it enters neither a difference's scatter nor the choice of "min")
            F, central = F - self._jac[None, :], central - self._jac
        B = F.shape[1]
        occ = np.flatnonzero(np.isfinite(central))
        if reference == "min":
            if not len(occ):
                raise ValueError("UmbrellaPMF.uncertainty: every bin is empty")
            ref = int(occ[np.argmin(central[occ])])
        elif isinstance(reference, (int, np.integer)) and not isinstance(reference, bool) and 0 <= int(reference) < B:
            ref = int(reference)
            if not np.isfinite(central[ref]):
                raise ValueError(f"UmbrellaPMF.uncertainty: the reference bin {ref} is empty")
        else:
            raise ValueError(f"reference {reference!r}: expected 'min' or a bin index in [0, {B})")
        out = np.full(B, np.nan)
        for b in range(B):
            both = np.isfinite(F[:, b]) & np.isfinite(F[:, ref])
            if both.sum() >= 2:
                out[b] = np.std(F[both, b] - F[both, ref], ddof=1)
        return torch.as_tensor(out, device=self.result.f.device)

    def uncertainty(self, reference="min", method: str = "asymptotic", weights=None) -> torch.Tensor:
        """(B,) float64 kJ/mol on the GPU: the standard deviation of F_b - F_ref of the unweighted profile ``pmf()``; 0 at the
        reference bin - "min": the occupied bin of lowest F, or a bin index - and NaN at an empty bin.  The Jacobian term is a
        constant and does not enter.  Each occupied bin is one more column x_n = e^{lw_n} / S_b on the bin's frames next to the
        windows' in the estimator's asymptotic covariance.
        ``method="bootstrap"`` (after ``fit(..., bootstrap=B)``): the sample standard deviation over the block-bootstrap
        replicates of F_b - F_ref, which holds for correlated frames and, with ``weights`` (N,), under DiffTRe weights.  A bin
        that is empty in a replicate is left out of that replicate's statistics; NaN where a bin (or the reference with it) is
        occupied in fewer than two replicates."""
        if method == "bootstrap":
            return self._boot_uncertainty(reference, weights)
        if method != "asymptotic":
            raise ValueError(f"method {method!r}: expected one of {ERROR_METHODS}")
        if weights is not None:
            raise ValueError("UmbrellaPMF.uncertainty: the asymptotic error bars hold at uniform weights; use method='bootstrap' with weights")
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

    def expect_error(self, values, method: str = "asymptotic", weights=None) -> torch.Tensor:
        """The standard deviation of ``result.expect(values)`` for ``values`` (N,) or (N, E): () or (E,) float64 on the GPU.  Two
        columns per observable, e^{lw} A' / sum e^{lw} A' with A' = A - min A + 1 > 0 and e^{lw} / sum e^{lw}:
        sigma^2 = <A'>^2 (Theta_AA + Theta_aa - 2 Theta_Aa).
        ``method="bootstrap"`` (after ``fit(..., bootstrap=B)``): the sample standard deviation over the replicates of
        sum_n m_bn w_n e^{lw_bn} A_n / sum_n m_bn w_n e^{lw_bn}, with ``weights`` w (N,) or uniform."""
        plan, f = self._fitted("expect_error")
        v = torch.as_tensor(values, device=f.device).to(torch.float64)
        if v.dim() not in (1, 2) or v.shape[0] != plan.N:
            raise ValueError(f"values must have shape ({plan.N},) or ({plan.N}, E)")
        if not bool(torch.isfinite(v).all()):
            raise ValueError("UmbrellaPMF.expect_error: non-finite values")
        if method == "bootstrap":
            plan, f, w = self._boot_weights("expect_error", weights)
            cols = v.reshape(plan.N, -1)
            if self._resample.n_boot < 2:
                raise ValueError("UmbrellaPMF.expect_error: fewer than two replicates")
            one = torch.ones(plan.N, 1, dtype=torch.float64, device=f.device) if w is None else w[:, None]
            out = np.zeros(cols.shape[1])
            for at in range(0, cols.shape[1], 7):  # seven observables and the normalisation per launch
                part = cols[:, at:at + 7]
                sums = self._boot_sums("expect_error", torch.cat([one, one * part], dim=1).contiguous(), False)[:, 0, :]
                out[at:at + part.shape[1]] = np.std(sums[:, 1:] / sums[:, :1], axis=0, ddof=1)
            return torch.as_tensor(out.reshape(tuple(v.shape[1:])), device=f.device)
        if method != "asymptotic":
            raise ValueError(f"method {method!r}: expected one of {ERROR_METHODS}")
        if weights is not None:
            raise ValueError("UmbrellaPMF.expect_error: the asymptotic error bars hold at uniform weights; use method='bootstrap' with weights")
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
