"""Melting temperature of a duplex from an umbrella-sampled trajectory, by histogram reweighting
(mythos/observables/melting_temp.py:15-173), with the reference's names.

The trajectory, sampled at ``sim_temperature`` under umbrella weights, is re-evaluated at every temperature of
``temperature_range`` - one ``energy_fn.map_kt`` call, which for oxDNA1 / oxDNA2 / oxRNA2 is one energy launch and one
Debye-Hueckel sweep launch instead of T energy calls - and the finite-size-corrected bound:unbound ratio curve is
interpolated to 0.5.  Everything after the energies is a handful of torch operations on the (T, F) tensor, on its device,
differentiable: autograd carries d(Tm)/d(E_t(f)) back into ``map_kt``.

``bind_states`` and ``umbrella_weights`` come from the energy file of an oxDNA run
(``mythos_amd.input.oxdna_energy.read_energy``) or from the frames themselves: column 0 of
``mythos_amd.observables.OrderParameters(op_file, energy_fn)(trajectory)`` and its ``weights``.

Not built: umbrella sampling or VMMC themselves.
"""

from __future__ import annotations

import dataclasses as dc
from typing import Any

import torch

from mythos_amd.utils.units import get_kt_from_c

TARGETS = {
    "SL_avg_6bp": get_kt_from_c(31.2),  # degrees
    "SL_avg_8bp": get_kt_from_c(48.2),  # degrees
    "SL_avg_12bp": get_kt_from_c(64.7),  # degrees
}


def _t(x, like: torch.Tensor | None = None) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x
    return torch.as_tensor(x, dtype=torch.float64, device=None if like is None else like.device)


def interp1d(x, y, x_new) -> torch.Tensor:
    """Piecewise-linear interpolation of (x, y) at ``x_new``, x sorted first (``jax_interp1d``, melting_temp.py:22-37:
    ``jnp.interp`` of the sorted arrays, constant beyond either end).  Differentiable in x, y and x_new."""
    x, y = _t(x), _t(y, _t(x))
    x_new = _t(x_new, x).to(x.dtype)
    order = torch.argsort(x)
    xs, ys = x[order], y[order]
    if xs.shape[0] == 1:
        return ys[0].expand(x_new.shape).clone()
    i = torch.clamp(torch.searchsorted(xs.detach(), x_new.detach().contiguous(), right=True), 1, xs.shape[0] - 1)
    dx, dy = xs[i] - xs[i - 1], ys[i] - ys[i - 1]
    safe = torch.where(dx == 0, torch.ones_like(dx), dx)
    f = torch.where(dx == 0, ys[i], ys[i - 1] + (x_new - xs[i - 1]) / safe * dy)
    f = torch.where(x_new < xs[0], ys[0], f)
    return torch.where(x_new > xs[-1], ys[-1], f)


def compute_finf(ratio) -> torch.Tensor:
    """Finite size correction to the bound:unbound ratio (melting_temp.py:40-42)."""
    ratio = _t(ratio)
    return 1 + 1 / (2 * ratio) - torch.sqrt((1 + 1 / (2 * ratio)) ** 2 - 1)


def find_melting_temp(temperatures, ratios) -> torch.Tensor:
    """The temperature at which the ratio curve is 0.5 (melting_temp.py:45-56)."""
    return interp1d(ratios, _t(temperatures, _t(ratios)), 0.5)


def compute_curve_width(temperatures, ratios) -> torch.Tensor:
    """Temperature separation between ratio 0.2 and ratio 0.8 (melting_temp.py:59-71)."""
    temperatures = _t(temperatures, _t(ratios))
    return interp1d(ratios, temperatures, 0.8) - interp1d(ratios, temperatures, 0.2)


def extrapolated_ratios(e0, et, kt_sim, kts, bind_states, umbrella_weights) -> torch.Tensor:
    """The host algebra of ``MeltingTemp.get_extrap_ratios`` as a function of the energies alone: ``e0`` (F,) at the
    simulation temperature ``kt_sim``, ``et`` (T, F) at the temperatures ``kts`` (T,), the ``bond`` order parameter and the
    umbrella weight of every frame -> the finite-size-corrected bound:unbound ratio at every temperature, (T,)
    (melting_temp.py:130-140).  The largest exponent of each temperature is subtracted before ``exp``: it cancels in the
    ratio."""
    et = _t(et)
    e0, kts = _t(e0, et).to(et), _t(kts, et).to(et)
    bind = torch.as_tensor(bind_states, device=et.device)
    weights = _t(umbrella_weights, et).to(et)
    expo = (e0 / kt_sim)[None, :] - et / kts[:, None]
    boltz_factor = torch.exp(expo - expo.detach().max(dim=1, keepdim=True).values)
    unbiased_counts = (1 / weights)[None, :] * boltz_factor
    zero = torch.zeros((), dtype=et.dtype, device=et.device)
    total_unbound = torch.where((bind == 0)[None, :], unbiased_counts, zero).sum(1)
    total_bound = torch.where((bind != 0)[None, :], unbiased_counts, zero).sum(1)
    return compute_finf(total_bound / total_unbound)


@dc.dataclass(frozen=True)
class MeltingTemp:
    """Melting temperature of a duplex from umbrella sampling (melting_temp.py:74-173): the temperature at which the
    concentration of duplexes is double that of single strands.

    ``sim_temperature``: the temperature the trajectory was sampled at, simulation units.  ``temperature_range``: the
    temperatures to extrapolate to.  ``energy_fn``: a ``ComposedEnergyFunction``.  ``sweep``: passed to
    ``energy_fn.map_kt`` (None: one fused sweep where it applies; "per_temperature": the reference's loop)."""

    sim_temperature: float
    temperature_range: Any
    energy_fn: Any
    sweep: str | None = None

    def __call__(self, trajectory, bind_states, umbrella_weights, opt_params) -> torch.Tensor:
        return self.get_melting_temperature(trajectory, bind_states, umbrella_weights, opt_params)

    def _range(self, like: torch.Tensor) -> torch.Tensor:
        return torch.as_tensor(self.temperature_range, dtype=torch.float64).detach().to(like.device)

    def get_extrap_ratios(self, trajectory, bind_states, umbrella_weights, opt_params) -> torch.Tensor:
        """Bound:unbound ratios at the extrapolated temperatures, (T,)."""
        fn = self.energy_fn.with_params(opt_params)
        energies_t0 = fn.map(trajectory)
        energies_tx = fn.map_kt(trajectory, self.temperature_range, sweep=self.sweep)
        return extrapolated_ratios(energies_t0, energies_tx, self.sim_temperature, self._range(energies_tx), bind_states, umbrella_weights)

    def get_melting_temperature(self, trajectory, bind_states, umbrella_weights, opt_params) -> torch.Tensor:
        ratios = self.get_extrap_ratios(trajectory, bind_states, umbrella_weights, opt_params)
        return find_melting_temp(self._range(ratios), ratios)

    def get_melting_curve(self, trajectory, bind_states, umbrella_weights, opt_params) -> tuple[torch.Tensor, torch.Tensor]:
        ratios = self.get_extrap_ratios(trajectory, bind_states, umbrella_weights, opt_params)
        return self._range(ratios), ratios

    def get_melting_curve_width(self, trajectory, bind_states, umbrella_weights, opt_params) -> torch.Tensor:
        ratios = self.get_extrap_ratios(trajectory, bind_states, umbrella_weights, opt_params)
        return compute_curve_width(self._range(ratios), ratios)
