"""MARTINI 2/3 energy functions with the reference's surface (mythos/energy/martini/base.py:46-208,
m2/lj.py:14-157, m2/bond.py:15-71, m2/angle.py:16-129, m3/angle.py:8-11), evaluated by the HIP kernels
of mythos_amd/csrc/martini.hip, and ``Coulomb`` - reaction-field electrostatics as the GROMACS runs of the reference's
MARTINI workflows use them, which the reference itself never evaluates.

    top = MartiniTopology.from_top("topol.top")
    lj = LJ.from_topology(topology=top, params=LJConfiguration(**lj_params))
    energies = lj.map(trajectory)            # trajectory.center (S, M, 3) nm, trajectory.box_size (S, 3)

Energies are differentiable through ``torch.autograd`` with respect to the positions (the kernel
returns dU/dpos) and with respect to every configuration value given as a torch tensor that requires
grad - the analogue of ``jax.grad`` over ``with_params`` in the reference: the kernel returns
dU/dsigma, dU/deps per type pair and dU/dk, dU/dr0 (dU/dtheta0) per bond (angle), and autograd carries
them through the table construction (symmetric type tables, named bonds, couplings).
"""

from __future__ import annotations

from typing import Any

import numpy as np
import torch

from mythos_amd.input.gromacs import MartiniTopology

LJ_SIGMA_PREFIX = "lj_sigma_"
LJ_EPSILON_PREFIX = "lj_epsilon_"
BOND_K_PREFIX = "bond_k_"
BOND_R0_PREFIX = "bond_r0_"
ANGLE_K_PREFIX = "angle_k_"
ANGLE_THETA0_PREFIX = "angle_theta0_"
EPSILON_R = "epsilon_r"
EPSILON_RF = "epsilon_rf"


class MartiniEnergyConfiguration:
    """Dictionary-backed parameters with couplings (mythos/energy/martini/base.py:135-208)."""

    def __init__(self, couplings: dict[str, list[str]] | None = None, **kwargs):
        self.couplings = couplings or {}
        targets = [v for vals in self.couplings.values() for v in vals]
        if len(targets) != len(set(targets)):
            raise ValueError("Parameters cannot appear in more than one coupling")
        self.reversed_couplings = {v: k for k, vals in self.couplings.items() for v in vals}
        self.params = {}
        for key, value in kwargs.items():
            if key in self.couplings:
                for sub in self.couplings[key]:
                    self.params[sub] = value
            elif key not in self.reversed_couplings:
                self.params[key] = value
        self.__post_init__()

    def __post_init__(self) -> None: ...

    def init_params(self) -> "MartiniEnergyConfiguration":
        return self

    @property
    def opt_params(self) -> dict:
        out = {}
        for key, value in self.params.items():
            out[self.reversed_couplings.get(key, key)] = value
        return out

    def __getitem__(self, key: str):
        if key in self.params:
            return self.params[key]
        if key in self.couplings:
            return self.params[self.couplings[key][0]]
        raise KeyError(f"Parameter '{key}' not found in configuration.")

    def __contains__(self, key: str) -> bool:
        return key in self.params or key in self.couplings

    def __or__(self, other):
        new = dict(self.params)
        new.update(other.params if isinstance(other, MartiniEnergyConfiguration) else other)
        return type(self)(couplings=self.couplings, **new)


class LJConfiguration(MartiniEnergyConfiguration):
    """``lj_sigma_A_B`` / ``lj_epsilon_A_B`` per bead-type pair (m2/lj.py:18-53)."""

    def __post_init__(self) -> None:
        bead_types = set()
        for p in self.params:
            if not p.startswith((LJ_SIGMA_PREFIX, LJ_EPSILON_PREFIX)):
                raise ValueError(f"Unexpected parameter {p} for LJConfiguration")
            bead_types.update(p.split("_")[2:4])
        self.bead_types = tuple(sorted(bead_types))

        self.sigmas = self.table("sigma").detach().numpy()
        self.epsilons = self.table("epsilon").detach().numpy()

    def table(self, prefix: str) -> torch.Tensor:
        """(T, T) float64 table of ``lj_<prefix>_A_B`` values; differentiable where a value is a tensor."""

        def get(a, b):
            v = self.params.get(f"lj_{prefix}_{a}_{b}", self.params.get(f"lj_{prefix}_{b}_{a}"))
            if v is None:
                raise ValueError(f"Missing LJ {prefix} parameter for pair {a}_{b} ({b}_{a})")
            return _as_scalar(v)

        return torch.stack([torch.stack([get(i, j) for j in self.bead_types]) for i in self.bead_types])


class BondConfiguration(MartiniEnergyConfiguration):
    """``bond_k_NAME`` / ``bond_r0_NAME`` pairs (m2/bond.py:18-31)."""

    def __post_init__(self) -> None:
        for p in self.params:
            if not p.startswith((BOND_K_PREFIX, BOND_R0_PREFIX)):
                raise ValueError(f"Unexpected parameter {p} for BondConfiguration")
        if len(self.params) == 0 or len(self.params) % 2 != 0:
            raise ValueError("BondConfiguration requires pairs of k and r0 parameters")


class AngleConfiguration(MartiniEnergyConfiguration):
    """``angle_k_NAME`` / ``angle_theta0_NAME`` pairs, theta0 in radians (m2/angle.py:19-32)."""

    def __post_init__(self) -> None:
        for p in self.params:
            if not p.startswith((ANGLE_K_PREFIX, ANGLE_THETA0_PREFIX)):
                raise ValueError(f"Unexpected parameter {p} for AngleConfiguration")
        if len(self.params) == 0 or len(self.params) % 2 != 0:
            raise ValueError("AngleConfiguration requires pairs of k and theta0 parameters")


class CoulombConfiguration(MartiniEnergyConfiguration):
    """``epsilon_r`` (relative permittivity inside the cut-off) and ``epsilon_rf`` (beyond it; 0 means infinity) of
    reaction-field Coulomb - the mdp keys of the same names; the defaults are those of the reference's MARTINI runs
    (data/templates/martini/m2/DMPC/*/md.mdp).  ``epsilon_r`` may be optimised while ``epsilon_rf`` is 0; charges are
    not parameters."""

    def __init__(self, couplings: dict[str, list[str]] | None = None, **kwargs):
        kwargs.setdefault(EPSILON_R, 15.0)
        kwargs.setdefault(EPSILON_RF, 0.0)
        super().__init__(couplings, **kwargs)

    def __post_init__(self) -> None:
        for p in self.params:
            if p not in (EPSILON_R, EPSILON_RF):
                raise ValueError(f"Unexpected parameter {p} for CoulombConfiguration")
        if isinstance(self.params[EPSILON_RF], torch.Tensor) and self.params[EPSILON_RF].requires_grad:
            raise ValueError("epsilon_rf is not optimisable")
        if not _num(self.params[EPSILON_R]) > 0 or _num(self.params[EPSILON_RF]) < 0:
            raise ValueError("CoulombConfiguration needs epsilon_r > 0 and epsilon_rf >= 0 (0: infinity)")
        er = self.params[EPSILON_R]
        if isinstance(er, torch.Tensor) and er.requires_grad and _num(self.params[EPSILON_RF]) != 0.0:
            # with a finite epsilon_rf the energy is no longer proportional to 1 / epsilon_r: k_rf depends on it too
            raise ValueError("epsilon_r can only be optimised with epsilon_rf = 0 (infinity)")

    @property
    def opt_params(self) -> dict:
        return {k: v for k, v in super().opt_params.items() if k != EPSILON_RF}


def _as_scalar(v) -> torch.Tensor:
    """A configuration value as a 0-dim float64 CPU tensor (keeps the autograd graph of a tensor value)."""
    if isinstance(v, torch.Tensor):
        return v.to(device="cpu", dtype=torch.float64).reshape(())
    return torch.tensor(float(v), dtype=torch.float64)


def _num(v) -> float:
    return float(v.detach()) if isinstance(v, torch.Tensor) else float(v)


_THETA_KEYS = ("sigma", "eps", "bond_k", "bond_r0", "angle_k", "angle_t0")


class _MartiniOp(torch.autograd.Function):
    """column of the kernel's [lj, bond, angle] energies; ``theta`` = the six parameter arrays (CPU float64),
    only used to route gradients: the system already holds their values."""

    @staticmethod
    def forward(ctx, pos, box, system, column, *theta):
        want_pos = pos.requires_grad
        e, g = system.energy(pos.detach(), box, grads=want_pos)
        ctx.single = pos.dim() == 2
        ctx.want_pos = want_pos
        need = [t is not None and t.requires_grad for t in theta]
        ctx.need = need
        pg = None
        if any(need):
            pg = system.param_grads(pos.detach(), box, lj=need[0] or need[1], bonds=need[2] or need[3],
                                    angles=need[4] or need[5])
        ctx.pg = pg
        ctx.save_for_backward(*([g] if want_pos else []))
        return e[..., column]

    @staticmethod
    def backward(ctx, g_out):
        gpos = None
        if ctx.want_pos:
            (g,) = ctx.saved_tensors
            scale = g_out.to(g.dtype)
            gpos = g * (scale if ctx.single else scale[:, None, None])
        gtheta = [None] * 6
        if ctx.pg is not None:
            w = g_out.reshape(-1).to(torch.float64)  # one weight per frame
            for k, key in enumerate(_THETA_KEYS):
                if ctx.need[k]:
                    pgk = ctx.pg[key]
                    gtheta[k] = (w.reshape(-1, *([1] * (pgk.dim() - 1))) * pgk).sum(0).cpu()
        return (gpos, None, None, None, *gtheta)


class MartiniEnergyFunction:
    """Base of the MARTINI terms (mythos/energy/martini/base.py:98-132).  A term evaluates ONLY its own
    contribution: the other two are given neutral parameters in the shared kernel launch."""

    column = 0
    angle_kind = 0

    def __init__(self, *, params: MartiniEnergyConfiguration, atom_types, atom_names, residue_names, angles,
                 bonded_neighbors, unbonded_neighbors=None, transform_fn=None, dtype=torch.float64):
        if unbonded_neighbors is not None:
            raise ValueError("MartiniEnergyFunction does not support user-input unbonded_neighbors.")
        self.params = params
        self.atom_types, self.atom_names, self.residue_names = tuple(atom_types), tuple(atom_names), tuple(residue_names)
        self.angles = np.asarray(angles, dtype=np.int32).reshape(-1, 3)
        self.bonded_neighbors = np.asarray(bonded_neighbors, dtype=np.int32).reshape(-1, 2)
        self.transform_fn = transform_fn
        self.dtype = dtype
        self._system = None

    @classmethod
    def from_topology(cls, topology: MartiniTopology, **kwargs) -> "MartiniEnergyFunction":
        return cls(atom_types=topology.atom_types, atom_names=topology.atom_names, residue_names=topology.residue_names,
                   angles=topology.angles, bonded_neighbors=topology.bonded_neighbors, **kwargs)

    @property
    def bond_names(self) -> tuple:
        return tuple(f"{self.residue_names[b[0]]}_{self.atom_names[b[0]]}_{self.atom_names[b[1]]}" for b in self.bonded_neighbors)

    @property
    def angle_names(self) -> tuple:
        return tuple(
            f"{self.residue_names[a[0]]}_{self.atom_names[a[0]]}_{self.atom_names[a[1]]}_{self.atom_names[a[2]]}" for a in self.angles
        )

    # -- parameter plumbing (reference EnergyFunction protocol) ---------------------------------------
    def with_params(self, *repl_dicts: dict, **repl_kwargs: Any) -> "MartiniEnergyFunction":
        new = self.params
        for d in repl_dicts:
            new = new | d
        new = new | repl_kwargs
        out = object.__new__(type(self))
        out.__dict__.update(self.__dict__)
        out.params = new.init_params()
        out._system = None
        return out

    def with_props(self, **kwargs) -> "MartiniEnergyFunction":
        out = object.__new__(type(self))
        out.__dict__.update(self.__dict__)
        out.__dict__.update(kwargs)
        out._system = None
        return out

    def opt_params(self) -> dict:
        return self.params.opt_params

    def params_dict(self, **_) -> dict:
        return dict(self.params.params)

    # -- kernel inputs -----------------------------------------------------------------------------------
    def _tables(self):
        """(types, sigma, eps, bond_k, bond_r0, angle_k, angle_t0): neutral values unless overridden."""
        n = len(self.atom_types)
        nb, na = len(self.bonded_neighbors), len(self.angles)
        return (np.zeros(n, np.int32), np.ones((1, 1)), np.zeros((1, 1)), np.zeros(nb), np.ones(nb), np.zeros(na), np.zeros(na))

    def _theta(self) -> tuple:
        """The six parameter arrays as CPU float64 tensors, in ``_THETA_KEYS`` order; the ones this term owns
        are built from ``self.params`` so gradients flow back to tensor-valued configuration entries."""
        _, sg, ep, bk, br, ak, at = self._tables()
        return tuple(torch.as_tensor(np.asarray(a, dtype=np.float64)) for a in (sg, ep, bk, br, ak, at))

    def _get_system(self, device):
        from mythos_amd.hip_system import MartiniSystem

        if self._system is None or self._system.device != device:
            t = self._tables()[0]
            sg, ep, bk, br, ak, at = (x.detach().numpy() for x in self._theta())
            self._system = MartiniSystem(t, sg, ep, self.bonded_neighbors, bk, br, self.angles, ak, at,
                                         angle_kind=self.angle_kind, dtype=self.dtype, device=device)
        return self._system

    def compute_energy(self, trajectory) -> torch.Tensor:
        if self.transform_fn is not None:
            trajectory = self.transform_fn(trajectory)
        pos = trajectory.center
        if not isinstance(pos, torch.Tensor) or pos.device.type != "cuda":
            raise ValueError("trajectory.center must be a CUDA/HIP tensor (no CPU fallback)")
        if trajectory.box_size is None:
            raise ValueError("MARTINI energy functions need trajectory.box_size")
        system = self._get_system(pos.device)
        return _MartiniOp.apply(pos.to(self.dtype), trajectory.box_size, system, self.column, *self._theta())

    __call__ = compute_energy

    def map(self, body_sequence) -> torch.Tensor:
        """Per-frame energies (n_states,): one launch over all frames (reference: lax.map, m2/lj.py:110-127)."""
        return self.compute_energy(body_sequence)


class LJ(MartiniEnergyFunction):
    """Shifted-cut-off Lennard-Jones over all non-bonded pairs (m2/lj.py:92-157)."""

    column = 0

    def _tables(self):
        t, _, _, bk, br, ak, at = super()._tables()
        idx = {name: i for i, name in enumerate(self.params.bead_types)}
        types = np.array([idx[a] for a in self.atom_types], dtype=np.int32)
        return types, self.params.sigmas, self.params.epsilons, bk, br, ak, at

    def _theta(self):
        base = super()._theta()
        return (self.params.table("sigma"), self.params.table("epsilon"), *base[2:])


class Bond(MartiniEnergyFunction):
    """Harmonic bonds 1/2 k (r - r0)^2 (m2/bond.py:44-71)."""

    column = 1

    def _tables(self):
        t, sg, ep, _, _, ak, at = super()._tables()
        k = np.array([_num(self.params[BOND_K_PREFIX + n]) for n in self.bond_names])
        r0 = np.array([_num(self.params[BOND_R0_PREFIX + n]) for n in self.bond_names])
        return t, sg, ep, k, r0, ak, at

    def _theta(self):
        base = super()._theta()
        k = torch.stack([_as_scalar(self.params[BOND_K_PREFIX + n]) for n in self.bond_names])
        r0 = torch.stack([_as_scalar(self.params[BOND_R0_PREFIX + n]) for n in self.bond_names])
        return (*base[:2], k, r0, *base[4:])


class Angle(MartiniEnergyFunction):
    """G96 cosine angles 1/2 k (cos theta - cos theta0)^2, MARTINI 2 (m2/angle.py:97-129)."""

    column = 2
    use_G96 = True  # noqa: N815 - reference spelling
    angle_kind = 0

    def _tables(self):
        t, sg, ep, bk, br, _, _ = super()._tables()
        k = np.array([_num(self.params[ANGLE_K_PREFIX + n]) for n in self.angle_names])
        t0 = np.array([_num(self.params[ANGLE_THETA0_PREFIX + n]) for n in self.angle_names])
        return t, sg, ep, bk, br, k, t0

    def _theta(self):
        base = super()._theta()
        k = torch.stack([_as_scalar(self.params[ANGLE_K_PREFIX + n]) for n in self.angle_names])
        t0 = torch.stack([_as_scalar(self.params[ANGLE_THETA0_PREFIX + n]) for n in self.angle_names])
        return (*base[:4], k, t0)


class Angle3(Angle):
    """Harmonic angles 1/2 k (theta - theta0)^2, MARTINI 3 (m3/angle.py:8-11)."""

    use_G96 = False  # noqa: N815
    angle_kind = 1


class _CoulombOp(torch.autograd.Function):
    """Reaction-field Coulomb energy per frame (mythos_martini_coulomb).  With epsilon_rf = 0 the energy is
    proportional to 1 / epsilon_r: dE/d(epsilon_r) = -E / epsilon_r, exact, on the host."""

    @staticmethod
    def forward(ctx, pos, box, system, eps_r):
        want_pos = pos.requires_grad
        e, g = system.coulomb(pos.detach(), box, grads=want_pos)
        ctx.single = pos.dim() == 2
        ctx.want_pos = want_pos
        ctx.save_for_backward(e, eps_r, *([g] if want_pos else []))
        return e

    @staticmethod
    def backward(ctx, g_out):
        e, eps_r, *rest = ctx.saved_tensors
        gpos = None
        if ctx.want_pos:
            scale = g_out.to(rest[0].dtype)
            gpos = rest[0] * (scale if ctx.single else scale[:, None, None])
        g_eps = None
        if ctx.needs_input_grad[3]:
            g_eps = (-(g_out.to(torch.float64) * e).sum() / eps_r.to(e.device)).to(eps_r.device).reshape(eps_r.shape)
        return gpos, None, None, g_eps


class Coulomb(MartiniEnergyFunction):
    """Reaction-field Coulomb between the charged beads, one cut-off with LJ (the system's ``r_cut``), potential shifted
    to zero there; bonded pairs carry the reaction-field part only, plus the constant self term (include/mythos_hip.h).
    The reference evaluates no Coulomb term - it leaves it to the GROMACS runs it drives - so this term has no
    counterpart in mythos/energy/martini; it makes `MartiniLangevinIntegrator` frames those of the GROMACS system."""

    def __init__(self, *, charges, **kwargs):
        super().__init__(**kwargs)
        if charges is None:
            raise ValueError("Coulomb needs per-bead charges (a topology read from a .top or .tpr carries them)")
        self.charges = np.ascontiguousarray(charges, dtype=np.float64)
        if self.charges.shape != (len(self.atom_types),):
            raise ValueError(f"charges must have shape ({len(self.atom_types)},)")

    @classmethod
    def from_topology(cls, topology: MartiniTopology, **kwargs) -> "Coulomb":
        kwargs.setdefault("params", CoulombConfiguration())
        return super().from_topology(topology, charges=topology.charges, **kwargs)

    def _get_system(self, device):
        fresh = self._system is None or self._system.device != device
        system = super()._get_system(device)
        if fresh:
            system.set_charges(self.charges, _num(self.params[EPSILON_R]), _num(self.params[EPSILON_RF]))
        return system

    def compute_energy(self, trajectory) -> torch.Tensor:
        if self.transform_fn is not None:
            trajectory = self.transform_fn(trajectory)
        pos = trajectory.center
        if not isinstance(pos, torch.Tensor) or pos.device.type != "cuda":
            raise ValueError("trajectory.center must be a CUDA/HIP tensor (no CPU fallback)")
        if trajectory.box_size is None:
            raise ValueError("MARTINI energy functions need trajectory.box_size")
        system = self._get_system(pos.device)
        return _CoulombOp.apply(pos.to(self.dtype), trajectory.box_size, system, _as_scalar(self.params[EPSILON_R]))

    __call__ = compute_energy


class MartiniComposedEnergyFunction:
    """Sum of MARTINI terms: the counterpart of ``ComposedEnergyFunction(energy_fns=..., strict_params=...)`` as the
    reference's MARTINI workflow builds it (examples/scripts/martini_full_reparameterization.py:147-154).
    ``with_params`` routes every key to the terms whose configuration holds it."""

    def __init__(self, energy_fns: list, strict_params: bool = True):
        if not isinstance(energy_fns, list) or not energy_fns or not all(isinstance(f, MartiniEnergyFunction) for f in energy_fns):
            raise TypeError("energy_fns must be a non-empty list of MartiniEnergyFunction terms")
        self.energy_fns = energy_fns
        self.strict_params = strict_params

    def _replace(self, energy_fns: list) -> "MartiniComposedEnergyFunction":
        return type(self)(energy_fns, strict_params=self.strict_params)

    def with_params(self, *repl_dicts: dict, **repl_kwargs: Any) -> "MartiniComposedEnergyFunction":
        repl = {k: v for d in repl_dicts for k, v in d.items()}
        repl.update(repl_kwargs)
        used, fns = set(), []
        for fn in self.energy_fns:
            own = {k: v for k, v in repl.items() if k in fn.params}
            used.update(own)
            fns.append(fn.with_params(**own) if own else fn)
        if self.strict_params and (unused := set(repl) - used):
            raise ValueError(f"Some parameters were not used in any energy function: {unused}.")
        return self._replace(fns)

    def with_props(self, **kwargs: Any) -> "MartiniComposedEnergyFunction":
        return self._replace([fn.with_props(**kwargs) for fn in self.energy_fns])

    def opt_params(self) -> dict:
        return {k: v for fn in self.energy_fns for k, v in fn.opt_params().items()}

    def params_dict(self, **kw) -> dict:
        return {k: v for fn in self.energy_fns for k, v in fn.params_dict(**kw).items()}

    def compute_energy(self, trajectory) -> torch.Tensor:
        total = self.energy_fns[0](trajectory)
        for fn in self.energy_fns[1:]:
            total = total + fn(trajectory)
        return total

    __call__ = compute_energy
    map = compute_energy


__all__ = [
    "Angle", "Angle3", "AngleConfiguration", "Bond", "BondConfiguration", "Coulomb", "CoulombConfiguration", "LJ", "LJConfiguration",
    "MartiniComposedEnergyFunction", "MartiniEnergyConfiguration", "MartiniEnergyFunction", "MartiniTopology",
]
