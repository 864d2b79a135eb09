r"""Membrane melting temperature (mythos/observables/membrane_melting_temp.py:27-220): the inflection of a sigmoid
fitted to area per lipid against temperature,

    APL(T) = apl0 + c_p_g T + dAPL sigmoid(k (T - Tm)),      parameters [apl0, c_p_g, dAPL, k, Tm].

The per-frame areas come from the membrane launch (``AreaPerLipid``); the weighted means per temperature are torch
reductions on the device; the fit - five unknowns, a dozen points - runs on the host in double.

The reference fits with jaxopt's LevenbergMarquardt and differentiates it implicitly.  Here the fit is a Marquardt loop
(damping scaled by diag(J^T J)) from the reference's initial guess, finished by Newton steps on grad_p 1/2 |r|^2 = 0 so
that the point returned is stationary to rounding.  Tm and the other parameters are differentiable with respect to the
areas by the implicit function theorem on that optimality condition, dp/dy = -H^-1 d(grad)/dy with the FULL Hessian
H = J^T J + sum_i r_i Hess(r_i): the Gauss-Newton J^T J alone is only right where the fitted residuals vanish
(DESIGN section 3.5c has the measured distances from finite differences).  The sigmoid is ``torch.sigmoid``: the literal
1 / (1 + exp(-k (T - Tm))) overflows from the initial guess, where k = 1.
"""

from __future__ import annotations

import dataclasses as dc

import numpy as np
import torch

from mythos_amd.input.gromacs import MartiniTopology
from mythos_amd.observables.membrane import AreaPerLipid


def _t(x):
    return x.to(torch.float64) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))


def calculate_apl(t, apl0, c_p_g, dAPL, k, Tm):  # noqa: N803 - the reference's names
    """The sigmoid model at temperature(s) ``t`` (K)."""
    t = _t(t)
    return apl0 + c_p_g * t + dAPL * torch.sigmoid(k * (t - Tm))


def apl_residual(coeffs, data):
    """``sim_apls - model`` for ``coeffs = [apl0, c_p_g, dAPL, k, Tm]`` and ``data = (sim_apls, sim_temps)``."""
    sim_apls, sim_temps = data
    apl0, c_p_g, dAPL, k, Tm = _t(coeffs)  # noqa: N806
    return _t(sim_apls) - calculate_apl(sim_temps, apl0, c_p_g, dAPL, k, Tm)


def get_initial_guess(sim_apls, sim_temps) -> torch.Tensor:
    """The reference's heuristic start (membrane_melting_temp.py:76-91)."""
    a, t = _t(sim_apls).detach(), _t(sim_temps).detach()
    return torch.stack([a.min() - 0.0001 * 276, torch.tensor(1e-4, dtype=torch.float64), a.max() - a.min(),
                        torch.tensor(1.0, dtype=torch.float64), torch.quantile(t, 0.5)])


def _model_and_jacobian(p, t):
    """f (n,) and df/dp (n, 5) in numpy."""
    a, c, d, k, m = p
    u = k * (t - m)
    s = np.where(u >= 0, 1.0 / (1.0 + np.exp(-np.abs(u))), np.exp(-np.abs(u)) / (1.0 + np.exp(-np.abs(u))))
    ds = s * (1.0 - s)
    return a + c * t + d * s, np.stack([np.ones_like(t), t, s, d * ds * (t - m), -d * ds * k], axis=1)


def _half_sq(p, y, t):
    r = apl_residual(p, (y, t))
    return 0.5 * torch.sum(r * r)


def _hessian(p, y, t) -> np.ndarray:
    """The full Hessian of 1/2 |r|^2 with respect to the parameters."""
    h = torch.autograd.functional.hessian(lambda q: _half_sq(q, torch.as_tensor(y), torch.as_tensor(t)), torch.as_tensor(p))
    return h.numpy()


def _solve_fit(y: np.ndarray, t: np.ndarray, maxiter: int) -> np.ndarray:
    p = get_initial_guess(y, t).numpy().copy()
    f, jac = _model_and_jacobian(p, t)
    r = y - f
    cost, lam = 0.5 * r @ r, 1e-3
    for _ in range(maxiter):
        g = -jac.T @ r  # gradient of the cost
        jtj = jac.T @ jac
        scale = np.maximum(np.diag(jtj), 1e-30)
        if np.max(np.abs(g) / np.sqrt(scale)) <= 1e-15 * max(np.sqrt(2.0 * cost), 1e-300):
            break
        try:
            step = np.linalg.solve(jtj + lam * np.diag(scale), -g)
        except np.linalg.LinAlgError:
            lam *= 10.0
            continue
        f_new, jac_new = _model_and_jacobian(p + step, t)
        r_new = y - f_new
        cost_new = 0.5 * r_new @ r_new
        if np.isfinite(cost_new) and cost_new <= cost:
            small = np.max(np.abs(step)) <= 1e-15 * max(1.0, np.max(np.abs(p)))
            p, r, jac, cost, lam = p + step, r_new, jac_new, cost_new, max(lam / 10.0, 1e-15)
            if small:
                break
        else:
            lam *= 10.0
            if lam > 1e30:
                break
    # Newton on the optimality condition: taken while it brings the gradient down
    for _ in range(8):
        f, jac = _model_and_jacobian(p, t)
        g = -jac.T @ (y - f)
        try:
            q = p - np.linalg.solve(_hessian(p, y, t), g)
        except np.linalg.LinAlgError:
            break
        f_q, jac_q = _model_and_jacobian(q, t)
        g_q = -jac_q.T @ (y - f_q)
        if not np.all(np.isfinite(g_q)) or np.linalg.norm(g_q) >= np.linalg.norm(g):
            break
        p = q
    return p


class _SigmoidFit(torch.autograd.Function):
    """Fitted parameters as a function of the areas; backward by the implicit function theorem, full Hessian."""

    @staticmethod
    def forward(ctx, sim_apls, sim_temps, maxiter):
        y, t = sim_apls.detach().cpu().numpy().astype(np.float64), sim_temps.detach().cpu().numpy().astype(np.float64)
        p = _solve_fit(y, t, maxiter)
        ctx.fit = (p, y, t)
        return torch.as_tensor(p).to(sim_apls.device)

    @staticmethod
    def backward(ctx, grad_p):
        p, y, t = ctx.fit
        _, jac = _model_and_jacobian(p, t)
        # grad = -F^T (y - f):  d grad / dy = -F^T,  dp/dy = H^-1 F^T,  so  dL/dy = F H^-1 dL/dp  (H symmetric)
        gy = jac @ np.linalg.solve(_hessian(p, y, t), grad_p.detach().cpu().numpy().astype(np.float64))
        return torch.as_tensor(gy).to(grad_p.device), None, None


def fit_apl_sigmoid(sim_apls, sim_temps, *, implicit_diff: bool = True, maxiter: int = 5000) -> torch.Tensor:
    """Fitted ``[apl0, c_p_g, dAPL, k, Tm]`` (float64, on the device of ``sim_apls``).

    With ``implicit_diff`` the result is differentiable with respect to ``sim_apls``.  Without it the reference
    differentiates the unrolled solver, which has no counterpart here: areas that require a gradient are then refused
    (``ValueError``) instead of silently yielding none; areas without one are fitted as usual."""
    y, t = _t(sim_apls), _t(sim_temps)
    if y.dim() != 1 or y.shape != t.shape:
        raise ValueError(f"sim_apls {tuple(y.shape)} and sim_temps {tuple(t.shape)} must be 1-D of one length")
    if not implicit_diff and y.requires_grad:
        raise ValueError("implicit_diff=False: differentiating the unrolled solver is not supported; use implicit_diff=True "
                         "or pass areas that do not require a gradient")
    return _SigmoidFit.apply(y, t, int(maxiter))


def compute_membrane_tm(sim_apls, sim_temps, *, implicit_diff: bool = True) -> torch.Tensor:
    """Tm (K) of the fit, a 0-d tensor."""
    return fit_apl_sigmoid(sim_apls, sim_temps, implicit_diff=implicit_diff)[4]


@dc.dataclass(frozen=True, kw_only=True)
class MembraneMeltingTemp:
    """Tm from a trajectory concatenated over simulations at several temperatures.

    Frames are grouped by ``trajectory.temperature`` within ``temp_rtol`` of each of ``temperatures``; the area per lipid
    of every frame comes from one membrane launch; each temperature's expected area is the mean weighted by ``weights``
    (DiffTRe weights; uniform if ``None``); Tm is that of the fitted sigmoid, differentiable with respect to ``weights``.
    Raises the reference's ValueErrors: no frames at a temperature, zero weight sum."""

    topology: MartiniTopology
    lipid_sel: str | tuple
    temperatures: object
    implicit_diff: bool = True
    temp_rtol: float = 1e-3

    def _apl(self) -> AreaPerLipid:
        fn = self.__dict__.get("_apl_fn")
        if fn is None:
            fn = AreaPerLipid(topology=self.topology, lipid_sel=self.lipid_sel)
            self.__dict__["_apl_fn"] = fn
        return fn

    def __call__(self, trajectory, weights=None) -> torch.Tensor:
        temps = _t(self.temperatures).reshape(-1)
        if getattr(trajectory, "temperature", None) is None:
            raise ValueError("MembraneMeltingTemp needs trajectory.temperature (per frame)")
        frame_t = torch.as_tensor(trajectory.temperature).detach().to("cpu", torch.float64).reshape(-1)
        groups = []  # the frames of each temperature, from the labels on the host: no device work yet
        for temp in temps.tolist():
            idx = torch.where((frame_t - temp).abs() < self.temp_rtol * abs(temp))[0]
            if idx.numel() == 0:
                raise ValueError(f"No frames found for temperature {temp} within relative tolerance {self.temp_rtol}.")
            groups.append(idx)
        apls = self._apl()(trajectory)
        if weights is None:
            weights = torch.ones(apls.shape[0], dtype=torch.float64, device=apls.device)
        weights = torch.as_tensor(weights).to(apls.device, torch.float64)
        groups = [idx.to(apls.device) for idx in groups]
        weight_sums = torch.stack([weights[idx].sum() for idx in groups])
        weighted = torch.stack([(weights[idx] * apls[idx]).sum() for idx in groups])
        # one read-back for the check; the fit reads the expected areas on the host anyway
        empty = torch.nonzero(weight_sums.detach().cpu() == 0)
        if empty.numel():
            temp = temps[int(empty[0])].item()
            raise ValueError(f"Sum of weights is zero for temperature {temp}. Cannot compute weighted average APL.")
        return compute_membrane_tm(weighted / weight_sums, temps, implicit_diff=self.implicit_diff)
