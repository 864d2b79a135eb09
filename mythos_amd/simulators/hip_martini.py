"""MARTINI simulator on the device-resident temperature ensemble: the counterpart of the reference's ``GromacsSimulator``
(mythos/simulators/gromacs/gromacs.py:70-131) as its MARTINI reparameterisation drives it, one run per simulation
temperature under one md.mdp (examples/scripts/martini_full_reparameterization.py:340-381) - here one
:class:`MartiniEnsembleIntegrator` whose replicas are the temperatures.

``run(opt_params, seed=...)`` lowers ``energy_fn.with_params(opt_params)`` to the tables of one ``MartiniSystem``, uploads
them into the resident handles (made at the first run and kept, as ``HipMDSimulator`` keeps its), equilibrates without
output, runs production and returns one ``SimulatorTrajectory`` per temperature, on the GPU.  ``restraints``: a
``MartiniRestraints`` set (mythos_amd.simulators.martini_restraints), repeated per temperature.  Not built: gradients
through the run, the restraints' bias as a term of the energy functions."""

from __future__ import annotations

import dataclasses as dc
from typing import Any

import numpy as np
import torch

from mythos_amd.simulators.base import Simulator, SimulatorOutput

KB = 0.0083144626  # kJ/mol/K

BAROSTAT_KEYS = ("kind", "coupling", "ref_p", "compressibility", "tau_p", "every")
_MDP_KEYS = {"pcoupl": "kind", "pcoupltype": "coupling", "ref-p": "ref_p", "ref_p": "ref_p", "compressibility": "compressibility",
             "tau-p": "tau_p", "tau_p": "tau_p", "nstpcouple": "every"}


def lower_martini(energy_fn) -> dict:
    """The tables of ONE ``MartiniSystem`` from the current parameters of a ``MartiniComposedEnergyFunction`` of LJ, Bond,
    Angle / Angle3 and optionally Coulomb: every term contributes the tables it owns, exactly as it hands them to its own
    system (``_tables`` for the types, ``_theta`` for the reals).  A single term (the stress profile of one term) stands for
    all three: it hands out neutral values for the tables it does not own, as it does to its own system."""
    from mythos_amd.energy import martini as M

    by = {}
    if isinstance(energy_fn, M.MartiniEnergyFunction):
        by = {"lj": energy_fn, "bond": energy_fn, "angle": energy_fn}
        if isinstance(energy_fn, M.Coulomb):
            by["coulomb"] = energy_fn
    else:
        fns = getattr(energy_fn, "energy_fns", None)
        if not fns:
            raise TypeError("energy_fn must be a MartiniComposedEnergyFunction or a single MARTINI term")
        for fn in fns:
            kind = "coulomb" if isinstance(fn, M.Coulomb) else "lj" if isinstance(fn, M.LJ) else "bond" if isinstance(fn, M.Bond) else \
                "angle" if isinstance(fn, M.Angle) else None
            if kind is None or kind in by:
                raise ValueError(f"energy_fn must hold one LJ, one Bond, one Angle / Angle3 and at most one Coulomb term, not {type(fn).__name__}"
                                 + (" twice" if kind else ""))
            by[kind] = fn
    missing = {"lj", "bond", "angle"} - set(by)
    if missing:
        raise ValueError(f"energy_fn lacks the terms {sorted(missing)}")
    real = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float64)  # noqa: E731
    lj, bond, angle = by["lj"], by["bond"], by["angle"]
    sg, ep = (real(t) for t in lj._theta()[:2])
    bk, br = (real(t) for t in bond._theta()[2:4])
    ak, at = (real(t) for t in angle._theta()[4:6])
    out = dict(types=np.asarray(lj._tables()[0], dtype=np.int32), sigma=sg, eps=ep, bonds=np.asarray(lj.bonded_neighbors, dtype=np.int32),
               bond_k=bk, bond_r0=br, angles=np.asarray(lj.angles, dtype=np.int32), angle_k=ak, angle_t0=at, angle_kind=int(angle.angle_kind),
               charges=None, epsilon_r=15.0, epsilon_rf=0.0)
    if "coulomb" in by:
        c = by["coulomb"]
        out.update(charges=np.asarray(c.charges, dtype=np.float64), epsilon_r=M._num(c.params[M.EPSILON_R]),
                   epsilon_rf=M._num(c.params[M.EPSILON_RF]))
    return out


def barostat_settings(barostat) -> dict | None:
    """``dict(kind=, coupling=, ref_p=, compressibility=, tau_p=, every=)`` for ``set_barostat`` from those keys or from
    the keys of an .mdp (pcoupl, pcoupltype, ref-p, compressibility, tau-p, nstpcouple; values may be the file's strings).
    ``None``, or pcoupl = no: no coupling."""
    if barostat is None:
        return None
    out = {}
    for k, v in dict(barostat).items():
        lk = str(k).lower()
        key = _MDP_KEYS.get(lk, _MDP_KEYS.get(lk.replace("_", "-"), lk))
        if key not in BAROSTAT_KEYS:
            raise ValueError(f"barostat: unknown key {k!r} (known: {BAROSTAT_KEYS} or the .mdp's {sorted(_MDP_KEYS)})")
        if isinstance(v, str):
            parts = v.split()
            if key in ("kind", "coupling"):
                v = parts[0].lower()
            else:
                nums = [float(p) for p in parts]
                v = nums[0] if len(nums) == 1 else tuple(nums)
        out[key] = v
    if out.get("kind") in (None, "no"):
        return None
    if out["kind"] not in ("berendsen", "c-rescale"):
        raise ValueError(f"barostat kind {out['kind']!r} is not built: 'berendsen' or 'c-rescale'")
    out.setdefault("coupling", "isotropic")
    if out["coupling"] not in ("isotropic", "semiisotropic"):
        raise ValueError(f"barostat coupling {out['coupling']!r} is not built: 'isotropic' or 'semiisotropic'")
    out["every"] = int(out.get("every", 10))
    out["tau_p"] = float(out.get("tau_p", 1.0))
    if out["every"] < 1 or not out["tau_p"] > 0:
        raise ValueError("barostat: every >= 1 and tau_p > 0 required")
    return out


def check_arguments(n: int, init_positions, box, temperatures, equilibration_steps, simulation_steps, save_every, barostat):
    """-> (temperatures (R,) K, positions (R, n, 3), boxes (R, 3), barostat settings), or ValueError; touches no device.
    Any cadence of ``save_every`` against the barostat's ``every`` is served, as by the single integrator (a row saved at a
    coupling step is the state before the event)."""
    from mythos_amd.hip_system import MartiniEnsembleIntegrator

    t = np.atleast_1d(np.asarray(temperatures, dtype=np.float64))
    if t.ndim != 1 or t.size < 1 or not np.all(np.isfinite(t)) or not np.all(t > 0):
        raise ValueError("temperatures must be a non-empty sequence of positive temperatures in K")
    r = int(t.size)
    x = np.asarray(init_positions, dtype=np.float64)
    if x.shape == (n, 3):
        x = np.broadcast_to(x, (r, n, 3))
    if x.shape != (r, n, 3):
        raise ValueError(f"init_positions must have shape ({n}, 3) or ({r}, {n}, 3) for {r} temperatures, not {tuple(np.shape(init_positions))}")
    boxes = MartiniEnsembleIntegrator.replica_boxes(box, r)
    if int(equilibration_steps) < 0 or int(simulation_steps) < 1 or int(save_every) < 1 or int(simulation_steps) % int(save_every):
        raise ValueError("equilibration_steps >= 0, and simulation_steps a positive multiple of save_every >= 1, required")
    return t, np.ascontiguousarray(x), boxes, barostat_settings(barostat)


@dc.dataclass(frozen=True, kw_only=True)
class HipMartiniSimulator(Simulator):
    """See the module docstring.  ``temperatures`` in K (one is R = 1 on the same path); ``save_every`` is the reference's
    ``nstxout``; ``neighbors = (skin, every)``; ``inner = (margin, every)`` or None; ``precision`` "float32" | "float64".
    ``exchange_every = E`` > 0: replica exchange between the temperatures every E steps, in equilibration and production
    (exchange seed ``seed + R``, next seed ``seed + R + 1``); ``observables[t]`` is then the trajectory of temperature t,
    gathered from the slots that held it, and ``state`` gains ``ladder`` and ``exchange``.
    ``restraints``: a ``MartiniRestraints`` set, the same for every temperature except where a pull coordinate's ``init`` /
    ``k`` hold (R,) values - ``temperatures=[T] * R`` with ``init`` of shape (R,) are R umbrella windows in one launch;
    references left None are the positions the run starts from.  ``state["pull"]`` is then the (rows, R, P) float64 tensor
    of the pull coordinates of the saved frames, on the GPU.  Refused with a barostat or exchange.
    ``window_exchange_every = E`` > 0 (with ``restraints`` and equal temperatures): Hamiltonian replica exchange between
    the windows every E steps, in equilibration and production (seeds as for ``exchange_every``); ``observables[w]`` and
    ``state["pull"][:, w]`` are then the trajectory of WINDOW w, gathered from the slots that held it, so that
    ``mbar_umbrella(state["pull"], restraints, kT)`` works unchanged; ``state`` gains ``windows`` (the slot-major
    assignment, taken up again by ``run(state=...)``) and ``window_exchange``.  Refused with
    ``exchange_every`` > 0 or a barostat."""

    energy_fn: Any
    topology: Any = None
    init_positions: Any
    box: Any
    temperatures: Any
    dt: float = 0.02
    gamma: float = 1.0
    masses: Any = None
    equilibration_steps: int = 0
    simulation_steps: int
    save_every: int
    neighbors: tuple = (0.5, 12)
    inner: tuple | None = None
    barostat: dict | None = None
    exchange_every: int = 0
    restraints: Any = None
    window_exchange_every: int = 0
    precision: str = "float32"
    device: Any = None
    _resident: dict = dc.field(default_factory=dict, repr=False, compare=False)

    def __post_init__(self):
        if self.precision not in ("float32", "float64"):
            raise ValueError("precision must be 'float32' or 'float64'")
        if int(self.exchange_every) < 0 or (int(self.exchange_every) > 0 and np.size(self.temperatures) < 2):
            raise ValueError("exchange_every >= 0, and at least two temperatures to exchange between, required")
        wx = int(self.window_exchange_every)
        if wx < 0 or (wx > 0 and (not self.restraints or np.size(self.temperatures) < 2)):
            raise ValueError("window_exchange_every >= 0, and restraints with at least two windows to exchange between, required")
        if wx > 0 and int(self.exchange_every) > 0:
            raise ValueError("window_exchange_every together with exchange_every is refused: exchange with different kT and windows is not built")
        if wx > 0 and barostat_settings(self.barostat):
            raise ValueError("window_exchange_every together with a barostat is refused: restraints under pressure coupling are not built")
        if wx > 0 and np.unique(np.asarray(self.temperatures, dtype=np.float64)).size != 1:
            raise ValueError("window_exchange_every needs every replica at the same temperature: exchange with different kT and windows is not built")
        if self.restraints and (barostat_settings(self.barostat) or int(self.exchange_every) > 0):
            raise ValueError("restraints together with a barostat or replica exchange are not built (the restraint virial, the "
                             "restraint energy in the exchange's H)")
        n = len(lower_martini(self.energy_fn)["types"])
        check_arguments(n, self.init_positions, self.box, self.temperatures, self.equilibration_steps, self.simulation_steps,
                        self.save_every, self.barostat)

    @property
    def systems_created(self) -> int:
        """How many ``MartiniSystem`` handles this simulator has made (one, however many runs)."""
        return self._resident.get("created", 0)

    def release(self) -> None:
        for key in ("integrator", "system"):
            h = self._resident.pop(key, None)
            if h is not None:
                h.close()

    def _handles(self, low, temps, baro, seed):
        from mythos_amd.hip_system import MartiniEnsembleIntegrator, MartiniSystem

        res = self._resident
        reals = tuple(low[k] for k in ("sigma", "eps", "bond_k", "bond_r0", "angle_k", "angle_t0"))
        if "system" not in res:
            dtype = torch.float32 if self.precision == "float32" else torch.float64
            res["system"] = MartiniSystem(low["types"], low["sigma"], low["eps"], low["bonds"], low["bond_k"], low["bond_r0"], low["angles"],
                                          low["angle_k"], low["angle_t0"], angle_kind=low["angle_kind"], dtype=dtype, device=self.device)
            res["created"] = res.get("created", 0) + 1
            integ = MartiniEnsembleIntegrator(res["system"], dt=self.dt, kT=KB * temps, gamma=self.gamma, mass=self.masses, seeds=seed)
            integ.set_neighbor_policy(*self.neighbors)
            if self.inner:
                integ.set_inner_list(*self.inner)
            if baro:
                integ.set_barostat(**baro)
            res["integrator"] = integ
        else:
            res["system"].set_params(*reals)
        if low["charges"] is not None:
            res["system"].set_charges(low["charges"], low["epsilon_r"], low["epsilon_rf"])
        return res["system"], res["integrator"]

    def run(self, opt_params: dict | None = None, *, seed: int = 0, state: dict | None = None, **_kwargs) -> SimulatorOutput:
        from mythos_amd.energy.base import Quaternion
        from mythos_amd.simulators.io import SimulatorTrajectory

        fn = self.energy_fn.with_params(opt_params) if opt_params else self.energy_fn
        low = lower_martini(fn)
        n = len(low["types"])
        temps, x0, boxes, baro = check_arguments(n, self.init_positions, self.box, self.temperatures, self.equilibration_steps,
                                                 self.simulation_steps, self.save_every, self.barostat)
        system, integ = self._handles(low, temps, baro, seed)
        r = len(temps)
        integ.restart([int(seed) + k for k in range(r)], 0)
        state = state or {}
        exchange = int(self.exchange_every)
        if exchange:  # equilibration and production both exchange; the decisions' seed follows the replicas'
            integ.set_exchange(exchange, int(seed) + r)
            if "ladder" in state:
                integ.set_ladder(np.asarray(state["ladder"]))
        pos = torch.as_tensor(state["positions"] if "positions" in state else x0).to(device=system.device, dtype=system.dtype).contiguous().clone()
        vel = (torch.as_tensor(state["velocities"]).to(device=system.device, dtype=system.dtype).contiguous().clone()
               if "velocities" in state else integ.init_velocities())
        windows = int(self.window_exchange_every)
        if windows:  # as for the temperatures: both phases exchange, the decisions' seed follows the replicas'
            integ.set_window_exchange(windows, int(seed) + r)
        if self.restraints or integ.restraints:  # (the references left None follow the state this run starts from)
            integ.set_restraints(self.restraints, reference_pos=pos, box=state.get("boxes", boxes), topology=self.topology)
        if windows and "windows" in state:  # (set_restraints has put window w into slot w)
            integ.set_windows(np.asarray(state["windows"]))
        integ.load(pos, vel, state.get("boxes", boxes))
        if self.equilibration_steps:
            integ.advance(int(self.equilibration_steps))
        traj, _ = integ.advance(int(self.simulation_steps), save_every=int(self.save_every), want_energy=False)
        lb = integ.last_boxes
        integ.store(pos, vel)
        if exchange:
            return self._exchanged_output(integ, traj, lb, temps, pos, vel, int(seed) + r + 1)
        if windows:
            return self._window_output(integ, traj, lb, temps, pos, vel, int(seed) + r + 1)
        s = traj.shape[0]
        q = torch.zeros((s, n, 4), dtype=traj.dtype, device=traj.device)
        q[..., 0] = 1.0
        out = [SimulatorTrajectory(center=traj[:, k].contiguous(), orientation=Quaternion(vec=q), box_size=lb[:, k].contiguous(),
                                   temperature=torch.full((s,), KB * float(temps[k]), dtype=torch.float64, device=traj.device))
               for k in range(r)]
        st = dict(positions=pos, velocities=vel, boxes=integ.box, seed=int(seed) + r)
        if self.restraints:
            st["pull"] = integ.pull_values(traj)
        return SimulatorOutput(observables=out, state=st)

    @staticmethod
    def _by_rung(rung_rows, traj, lb, temps):
        """Slot-major rows -> one trajectory per rung: frame k of rung t is the slot that held t at row k, with that slot's
        box.  -> (trajectories, slot_of_rung (S, R))."""
        from mythos_amd.energy.base import Quaternion
        from mythos_amd.simulators.io import SimulatorTrajectory

        s, r, n = traj.shape[0], traj.shape[1], traj.shape[2]
        slot_of_rung = torch.argsort(rung_rows, dim=1)  # (S, R): the inverse of each row's permutation
        rows = torch.arange(s, device=traj.device)
        q = torch.zeros((s, n, 4), dtype=traj.dtype, device=traj.device)
        q[..., 0] = 1.0
        out = [SimulatorTrajectory(center=traj[rows, slot_of_rung[:, k]].contiguous(), orientation=Quaternion(vec=q),
                                   box_size=lb[rows, slot_of_rung[:, k]].contiguous(),
                                   temperature=torch.full((s,), KB * float(temps[k]), dtype=torch.float64, device=traj.device))
               for k in range(r)]
        return out, slot_of_rung

    def _window_output(self, integ, traj, lb, temps, pos, vel, next_seed) -> SimulatorOutput:
        """``observables[w]`` and ``state["pull"][:, w]`` are the trajectory OF WINDOW w, gathered as ``_exchanged_output``
        gathers the temperatures; xi depends on the configuration alone, so it is evaluated slot-major and gathered.  The
        state stays slot-major and gains the assignment."""
        out, slot_of_window = self._by_rung(integ.last_windows, traj, lb, temps)
        rows = torch.arange(traj.shape[0], device=traj.device)
        pull = integ.pull_values(traj)
        pull = torch.stack([pull[rows, slot_of_window[:, k]] for k in range(traj.shape[1])], dim=1).contiguous()
        attempts, accepts = integ.window_exchange_counts()
        return SimulatorOutput(observables=out, state=dict(positions=pos, velocities=vel, boxes=integ.box, seed=next_seed, pull=pull,
                                                           windows=integ.windows, window_exchange=dict(attempts=attempts, accepts=accepts)))

    def _exchanged_output(self, integ, traj, lb, temps, pos, vel, next_seed) -> SimulatorOutput:
        """``observables[t]`` is the trajectory OF TEMPERATURE t: frame k is the slot that held rung t at row k, with that
        slot's box; gathered on the GPU.  The state stays slot-major and gains the ladder."""
        out, _ = self._by_rung(integ.last_ladder, traj, lb, temps)
        attempts, accepts = integ.exchange_counts()
        return SimulatorOutput(observables=out, state=dict(positions=pos, velocities=vel, boxes=integ.box, seed=next_seed, ladder=integ.ladder,
                                                           exchange=dict(attempts=attempts, accepts=accepts)))
