r"""Extensible worm-like-chain fit of a force-extension curve (mythos/observables/wlc.py:9-103): Odijk's

    x(F) = L0 (1 + F / K - kT / (2 F L0) (1 + y coth y)),      y = (F L0^2 / (Lp kT))^(1/2),

fitted for ``[L0, Lp, K]`` - contour length, persistence length, stretch modulus - to the mean extensions measured
at several pulling forces (``ExtensionZ`` of runs with ``HipMDSimulator(external_forces=...)``).

The reference fits with jaxopt's GaussNewton and differentiates it implicitly.  Here the fit is a Gauss-Newton loop on
the host in double from the given start, finished by Newton steps on grad_p 1/2 |r|^2 = 0 so that the point returned is
stationary to rounding; the result is differentiable with respect to ``extensions`` by the implicit function theorem on
that optimality condition with the FULL Hessian H = J^T J + sum_i r_i Hess(r_i), as membrane_melting_temp.py does it
and for the reason given there: J^T J alone is only right where the fitted residuals vanish (DESIGN section 3.5d has
both distances from finite differences).
"""

from __future__ import annotations

import numpy as np
import torch


def _t(x):
    return x.to(torch.float64) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))


def coth(x):
    """Hyperbolic cotangent, the reference's literal form."""
    x = _t(x)
    return (torch.exp(2 * x) + 1) / (torch.exp(2 * x) - 1)


def calculate_extension(force, l0, lp, k, kT):  # noqa: N803 - the reference's names
    """Extension under ``force`` of an extensible worm-like chain (Odijk)."""
    force, l0, lp, k = _t(force), _t(l0), _t(lp), _t(k)
    y = ((force * l0**2) / (lp * kT)) ** 0.5
    return l0 * (1 + force / k - kT / (2 * force * l0) * (1 + y * coth(y)))


def loss(coeffs, extensions, forces, kT):  # noqa: N803
    """Residuals ``extensions - model`` for ``coeffs = [L0, Lp, K]``."""
    coeffs = _t(coeffs)
    return _t(extensions) - calculate_extension(forces, coeffs[0], coeffs[1], coeffs[2], kT)


def _model_and_jacobian(p: np.ndarray, f: np.ndarray, kT: float):  # noqa: N803
    """Model extensions (n,) and d(model)/dp (n, 3) in numpy (autograd in double on the host)."""
    with torch.enable_grad():  # (called from inside an autograd.Function, where recording is off)
        pt = torch.as_tensor(p, dtype=torch.float64).clone().requires_grad_(True)
        ft = torch.as_tensor(f, dtype=torch.float64)
        x = calculate_extension(ft, pt[0], pt[1], pt[2], kT)
        jac = torch.stack([torch.autograd.grad(x[i], pt, retain_graph=True)[0] for i in range(x.shape[0])])
    return x.detach().numpy(), jac.numpy()


def _hessian(p, y, f, kT, full: bool = True) -> np.ndarray:  # noqa: N803
    """Hessian of 1/2 |r|^2 with respect to the parameters: the full one, or the Gauss-Newton J^T J."""
    if not full:
        _, jac = _model_and_jacobian(p, f, kT)
        return jac.T @ jac
    yt, ft = torch.as_tensor(y, dtype=torch.float64), torch.as_tensor(f, dtype=torch.float64)
    with torch.enable_grad():
        h = torch.autograd.functional.hessian(lambda q: 0.5 * torch.sum(loss(q, yt, ft, kT) ** 2), torch.as_tensor(p, dtype=torch.float64))
    return h.numpy()


def _solve_fit(y: np.ndarray, f: np.ndarray, p0: np.ndarray, kT: float, maxiter: int) -> np.ndarray:  # noqa: N803
    p = p0.astype(np.float64).copy()
    for _ in range(maxiter):
        x, jac = _model_and_jacobian(p, f, kT)
        step = np.linalg.lstsq(jac, y - x, rcond=None)[0]
        if not np.all(np.isfinite(step)):
            break
        p = p + step
        if np.max(np.abs(step) / np.maximum(np.abs(p), 1e-300)) <= 1e-13:
            break
    # Newton on the optimality condition: taken while it brings the gradient down
    for _ in range(8):
        x, jac = _model_and_jacobian(p, f, kT)
        g = -jac.T @ (y - x)
        try:
            q = p - np.linalg.solve(_hessian(p, y, f, kT), g)
        except np.linalg.LinAlgError:
            break
        x_q, jac_q = _model_and_jacobian(q, f, kT)
        g_q = -jac_q.T @ (y - x_q)
        if not np.all(np.isfinite(g_q)) or np.linalg.norm(g_q) >= np.linalg.norm(g):
            break
        p = q
    return p


class _WlcFit(torch.autograd.Function):
    """Fitted parameters as a function of the extensions; backward by the implicit function theorem."""

    @staticmethod
    def forward(ctx, extensions, forces, init_guess, kT, maxiter, full_hessian):  # noqa: N803
        y = extensions.detach().cpu().numpy().astype(np.float64)
        f = forces.detach().cpu().numpy().astype(np.float64)
        p = _solve_fit(y, f, init_guess.detach().cpu().numpy().astype(np.float64), kT, maxiter)
        ctx.fit = (p, y, f, kT, full_hessian)
        return torch.as_tensor(p).to(extensions.device)

    @staticmethod
    def backward(ctx, grad_p):
        p, y, f, kT, full = ctx.fit  # noqa: N806
        _, jac = _model_and_jacobian(p, f, kT)
        # grad = -J^T (y - x(p)):  d grad / dy = -J^T,  dp/dy = H^-1 J^T,  so  dL/dy = J H^-1 dL/dp  (H symmetric)
        gy = jac @ np.linalg.solve(_hessian(p, y, f, kT, full), grad_p.detach().cpu().numpy().astype(np.float64))
        return torch.as_tensor(gy).to(grad_p.device), None, None, None, None, None


def fit_wlc(extensions, forces, init_guess, kT, *, implicit_diff: bool = True, maxiter: int = 200, full_hessian: bool = True) -> torch.Tensor:  # noqa: N803
    """Fitted ``[L0, Lp, K]`` (float64, on the device of ``extensions``), differentiable with respect to ``extensions``.

    ``implicit_diff=False`` (the reference then differentiates the unrolled solver, which has no counterpart here)
    refuses extensions that require a gradient instead of silently yielding none.  ``full_hessian=False`` uses the
    Gauss-Newton J^T J in the backward pass (what the tests measure the full Hessian against)."""
    y, f, p0 = _t(extensions), _t(forces), _t(init_guess)
    if y.dim() != 1 or y.shape != f.shape or p0.shape != (3,):
        raise ValueError(f"extensions {tuple(y.shape)} and forces {tuple(f.shape)} must be 1-D of one length, init_guess (3,)")
    if not implicit_diff and y.requires_grad:
        raise ValueError("implicit_diff=False: differentiating the unrolled solver is not supported; use implicit_diff=True "
                         "or pass extensions that do not require a gradient")
    return _WlcFit.apply(y, f, p0, float(kT), int(maxiter), bool(full_hessian))
