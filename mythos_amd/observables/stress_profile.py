"""Lateral pressure profile P(z) and surface tension of stored MARTINI frames, evaluated by the HIP library for every frame
of a trajectory in one call (mythos_amd/csrc/stress_profile.hip, ``mythos_martini_stress_profile``).

    sp = StressProfile(topology=top, energy_fn=energy_fn, n_bins=100, center="name C3A C3B")
    p = sp(trajectory)            # (S, n_bins, 3) P_xx, P_yy, P_zz in bar, float64 on the GPU
    pl = sp.lateral(trajectory)   # (S, n_bins) P_zz of the frame - 1/2 (P_xx + P_yy)(slab): integrates to the surface tension
    z, rho = sp.z(trajectory), sp.density(trajectory)   # slab centres (nm), bead density (nm^-3)
    gamma = SurfaceTension(topology=top, energy_fn=energy_fn)(trajectory) * to_mN_per_m   # (S,) mN/m
    expected = weights @ p.reshape(len(weights), -1)    # the reweighted profile of DiffTRe; differentiable in the weights

Definitions.  Every bead gets a share of the frame's diagonal virial, the decomposition of
``MartiniLangevinIntegrator.pressure`` term for term: an LJ pair, a bond, a reaction-field pair and an excluded
reaction-field pair give -1/2 (dV/dr) / r dx_d^2 to either bead, an angle -u_d dU/dx_id to its first and -v_d dU/dx_kd to its
last bead and nothing to its centre, all over minimum-image vectors.  The share sits at the bead's own z - a Harasima-type
contour.  Its lateral components are what the profile is for; **P_zz(z) of this contour is not constant in z, only its sum
over the slabs (``total``) is physical**, which is why ``lateral`` and the surface tension use the frame's total P_zz.

Slabs: ``n_bins`` of equal thickness Lz_f / n_bins of the frame's own box, so they follow the box under NPT.  With
``center=None`` they are fixed to the box, slab 0 starting at z = 0 (stored coordinates are wrapped into the box first).  With
``center=<selection>`` the profile is centred on the frame's midpoint, the mean stored z of the selection's beads - the
midpoint of ``MembraneThickness``, and like it wrong for a bilayer that lies across the z boundary of the stored
coordinates -; slab ``n_bins // 2`` then starts at the midplane.  Slab indices are computed in double from the stored
values, so an fp32 trajectory lands in the slabs of its fp64 copy.

Kinetic part: stored frames hold no velocities; a slab's kinetic part is its equipartition value n_b kT_f in every
direction, kT_f from ``kT=`` or else ``trajectory.temperature`` (kJ/mol).  P_d(b) = (n_b kT + W_d(b)) / (Lx Ly dz) x 16.6053907 bar.

Surface tension: gamma_f = sum_b dz_f [P_zz(b) - 1/2 (P_xx(b) + P_yy(b))] = Lz (P_zz - 1/2 (P_xx + P_yy)) of the frame's
totals, in bar nm (``to_mN_per_m`` = 0.1); it depends on neither the contour nor ``center``.

Per frame these are fixed vectors.  Their values depend on the energy function's parameters (the system is lowered from
``energy_fn`` as ``HipMartiniSimulator`` lowers it, under its current parameters and charges), but **no gradient with
respect to them is handed out**: a DiffTRe loss on the profile or on gamma gets the reweighting term only, as with
``OrderParameters``.  Not built: dP/dtheta of the per-frame values; the Irving-Kirkwood contour and the central-force
decomposition of angles it needs; off-diagonal components; profiles along x or y; the profile inside the step launch;
velocities for the kinetic term.
"""

from __future__ import annotations

import dataclasses as dc
from typing import Any

import numpy as np
import torch

from mythos_amd import _lib
from mythos_amd.hip_system import MartiniSystem, martini_frames
from mythos_amd.observables.membrane import select

MAX_BINS = _lib.STRESS_MAX_BINS
TERMS = ("kinetic", "lj", "bond", "angle", "coulomb")  # the fourth axis of a by_term profile
to_mN_per_m = 0.1  # noqa: N816 - 1 bar nm = 1e5 Pa x 1e-9 m = 0.1 mN/m


def bar_per_kj_mol_nm3() -> float:
    """kJ mol^-1 nm^-3 -> bar, the library's constant (the one the barostat uses)."""
    return float(_lib.load().mythos_martini_bar_per_kj_mol_nm3())


class _Stress:
    """What StressProfile and SurfaceTension share: the lowered system per precision and device, the launch, the units."""

    def _n_bins(self) -> int:
        raise NotImplementedError

    def _plan(self):
        """(tables, centre indices or None), built once on the host; raises the ValueErrors of the arguments."""
        cached = self.__dict__.get("_cached_plan")
        if cached is None:
            n_bins = self._n_bins()
            if int(n_bins) != n_bins or not 1 <= n_bins <= MAX_BINS:
                raise ValueError(f"n_bins {n_bins!r}: expected an integer in [1, {MAX_BINS}]")
            from mythos_amd.simulators.hip_martini import lower_martini

            low = lower_martini(self.energy_fn)  # (a composed function, or a single term with neutral values for the others)
            if len(low["types"]) != len(self.topology.atom_names):
                raise ValueError(f"energy_fn has {len(low['types'])} beads, the topology {len(self.topology.atom_names)}")
            center = getattr(self, "center", None)
            index = None if center is None else np.flatnonzero(select(self.topology, center)).astype(np.int32)
            cached = (low, index)
            self.__dict__["_cached_plan"] = cached
        return cached

    def __post_init__(self):
        self._plan()

    def _system(self, dtype, device) -> MartiniSystem:
        low = self._plan()[0]

        def make():
            s = MartiniSystem(low["types"], low["sigma"], low["eps"], low["bonds"], low["bond_k"], low["bond_r0"], low["angles"],
                              low["angle_k"], low["angle_t0"], angle_kind=low["angle_kind"], dtype=dtype, device=device)
            if low["charges"] is not None:
                s.set_charges(low["charges"], low["epsilon_r"], low["epsilon_rf"])
            return s

        return _lib.per_device(self, (dtype, device), make)

    def _rows(self, trajectory, by_term: bool):
        """-> (raw rows (S, n_bins, C) float64, box (S, 3) float64, kT (S,) float64), on the trajectory's device."""
        pos, box = martini_frames(trajectory.center, getattr(trajectory, "box_size", None))
        n = len(self.topology.atom_names)
        if pos.shape[1] != n:
            raise ValueError(f"trajectory has {pos.shape[1]} beads, the topology {n}")
        kT = self.kT if self.kT is not None else getattr(trajectory, "temperature", None)
        if kT is None:
            raise ValueError("the kinetic part of the pressure needs kT: neither trajectory.temperature nor kT= is given")
        kT = torch.as_tensor(kT, dtype=torch.float64, device=pos.device).reshape(-1)
        if kT.numel() not in (1, pos.shape[0]):
            raise ValueError(f"kT has {kT.numel()} values for {pos.shape[0]} frames")
        raw = self._system(pos.dtype, pos.device).stress_profile(pos, box, self._n_bins(), self._plan()[1], by_term=by_term,
                                                                 check_boxes=bool(self.check_boxes))
        return raw, box.to(torch.float64), kT.expand(pos.shape[0])

    def raw(self, trajectory) -> torch.Tensor:
        """(S, n_bins, 4) float64: bead count, W_x, W_y, W_z (kJ/mol) of every slab; with ``by_term`` (S, n_bins, 13): the
        count, then W of lj, bond, angle, coulomb (zero for an uncharged system)."""
        return self._rows(trajectory, bool(getattr(self, "by_term", False)))[0]

    def _pressures(self, trajectory, by_term: bool) -> tuple:
        """-> (P (S, n_bins, 3) or (S, n_bins, 5, 3) in bar, raw rows, box)."""
        raw, box, kT = self._rows(trajectory, by_term)
        nb = raw.shape[1]
        per_volume = bar_per_kj_mol_nm3() * nb / (box[:, 0] * box[:, 1] * box[:, 2])  # bar per kJ/mol in a slab of the frame
        kin = (raw[:, :, 0] * kT[:, None])[:, :, None].expand(-1, -1, 3)
        if by_term:
            parts = torch.cat([kin[:, :, None, :], raw[:, :, 1:].reshape(raw.shape[0], nb, 4, 3)], dim=2)
            return parts * per_volume[:, None, None, None], raw, box
        return (kin + raw[:, :, 1:4]) * per_volume[:, None, None], raw, box


@dc.dataclass(frozen=True, kw_only=True)
class StressProfile(_Stress):
    """``(S, n_bins, 3)`` P_xx, P_yy, P_zz per slab in bar; with ``by_term`` ``(S, n_bins, 5, 3)``: the kinetic part and the
    lj, bond, angle and coulomb parts (``TERMS``).  ``energy_fn``: a ``MartiniComposedEnergyFunction`` or a single term;
    ``center``: None or a selection of ``observables.membrane.select``; ``kT`` (kJ/mol): a number or one per frame, else
    ``trajectory.temperature``; ``check_boxes=False`` skips the box-edge check of every call and with it the call's one host
    synchronisation (for boxes already validated).  See the module docstring; no gradient with respect to the parameters is
    handed out."""

    topology: Any
    energy_fn: Any
    n_bins: int
    center: Any = None
    by_term: bool = False
    kT: Any = None  # noqa: N815
    check_boxes: bool = True

    def _n_bins(self) -> int:
        return self.n_bins

    def __call__(self, trajectory) -> torch.Tensor:
        return self._pressures(trajectory, bool(self.by_term))[0]

    def total(self, trajectory) -> torch.Tensor:
        """(S, 3) bar: the diagonal pressure of the stored frames, (n kT + W_d) / V - the sum over the slabs."""
        p = self._pressures(trajectory, False)[0]
        return p.sum(1) / p.shape[1]

    def lateral(self, trajectory) -> torch.Tensor:
        """(S, n_bins) bar: P_zz of the frame minus 1/2 (P_xx + P_yy) of the slab; sum_b dz lateral[b] is the surface tension."""
        p = self._pressures(trajectory, False)[0]
        return (p[:, :, 2].sum(1) / p.shape[1])[:, None] - 0.5 * (p[:, :, 0] + p[:, :, 1])

    def density(self, trajectory) -> torch.Tensor:
        """(S, n_bins) nm^-3: beads per volume of the slab."""
        raw, box, _ = self._rows(trajectory, False)
        return raw[:, :, 0] * raw.shape[1] / (box[:, 0] * box[:, 1] * box[:, 2])[:, None]

    def z(self, trajectory) -> torch.Tensor:
        """(S, n_bins) nm: slab centres, from the box origin (``center=None``) or from the midplane."""
        _, box = martini_frames(trajectory.center, getattr(trajectory, "box_size", None))
        nb = int(self.n_bins)
        frac = (torch.arange(nb, dtype=torch.float64, device=box.device) + 0.5) / nb - (0.0 if self.center is None else 0.5)
        return box[:, 2].to(torch.float64)[:, None] * frac[None, :]


@dc.dataclass(frozen=True, kw_only=True)
class SurfaceTension(_Stress):
    """``(S,)`` gamma_f = Lz (P_zz - 1/2 (P_xx + P_yy)) of the frame's totals in bar nm (times ``to_mN_per_m`` for mN/m).
    See the module docstring; no gradient with respect to the parameters is handed out."""

    topology: Any
    energy_fn: Any
    kT: Any = None  # noqa: N815
    check_boxes: bool = True

    def _n_bins(self) -> int:
        return 1

    def __call__(self, trajectory) -> torch.Tensor:
        p, _, box = self._pressures(trajectory, False)
        return box[:, 2] * (p[:, 0, 2] - 0.5 * (p[:, 0, 0] + p[:, 0, 1]))
