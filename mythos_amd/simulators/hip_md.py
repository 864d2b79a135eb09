"""MD sampler on the fused HIP Langevin kernel, shaped like the reference's ``JaxMDSimulator``
(mythos/simulators/jax_md/jaxmd.py:20-103) and ``StaticSimulatorParams``
(mythos/simulators/jax_md/utils.py:129-159).

    sim = HipMDSimulator(energy_fn=..., simulator_params=..., space=space.free(),
                         simulator_init=nvt_langevin, neighbors=NoNeighborList(top.unbonded_neighbors))
    out = sim.run(opt_params, init_state, n_steps, key)      # SimulatorOutput([SimulatorTrajectory])

The reference scans ``step_fn`` and stores the state after EVERY step - ``state.position`` and nothing else
(jaxmd.py:84-99); ``run`` does the same by default (``save_every=1``, positions only: the step launch that produces a
saved state writes it to its row, no other cost) but takes a cadence, and the whole loop is one C-ABI call.
``trace_energy=True`` adds the term and kinetic energies of the saved steps (``metadata``), at the price of the
energy-trace instantiation of the step kernel; the reference's way to the energies of a trajectory is ``energy_fn.map``.

The device-side objects of a run - the system handle with its neighbour rows, the integrator with its frames - are kept
on the simulator between calls, keyed by everything they were built from (topology, model, precision, device, replica
count, list, integrator constants).  A later ``run`` with other parameters uploads the 2 KB parameter vector, sets the
key and the step counter, and steps (the reference: "parameter update: negligible", docs/source/energy_functions.rst:51-54;
its own run re-traces nothing when only ``opt_params`` change, jaxmd.py:60-68).
"""

from __future__ import annotations

import dataclasses as dc
from typing import Any, Callable

import numpy as np
import torch

from mythos_amd.energy.base import ComposedEnergyFunction, EnergyFunction, Quaternion, RigidBody, _pairs_2xP, pair_tag, topology_key
from mythos_amd.energy.lowering import lower
from mythos_amd.hip_system import LangevinIntegrator, OxdnaSystem
from mythos_amd.input.external_forces import read_external_field, read_external_forces
from mythos_amd.simulators.base import Simulator, SimulatorOutput
from mythos_amd.simulators.io import SimulatorTrajectory
from mythos_amd.simulators.replicas import ReplicaLayout
from mythos_amd.simulators.neighbors import NoNeighborList, VerletNeighborList  # noqa: F401  (NoNeighborList: re-exported, the docstring's example)


@dc.dataclass
class StaticSimulatorParams:
    """mythos/simulators/jax_md/utils.py:129-159.  ``mass`` / ``gamma`` are RigidBody-shaped in the
    reference (center = translational, orientation = rotational); here plain pairs."""

    seq: Any
    mass: Any  # RigidBody(center=m, orientation=(I1, I2, I3)) or (m, (I1, I2, I3))
    gamma: Any  # RigidBody(center=gamma_t, orientation=gamma_r) or (gamma_t, gamma_r)
    bonded_neighbors: Any
    checkpoint_every: int
    dt: float
    kT: float  # noqa: N815

    @property
    def sim_init_fn(self) -> dict:
        return {"dt": self.dt, "kT": self.kT, "gamma": self.gamma}

    @property
    def init_fn(self) -> dict:
        return {"mass": self.mass}

    @property
    def step_fn(self) -> dict:
        return {}


def _pair(x):
    if isinstance(x, RigidBody):
        return x.center, x.orientation
    return x


@dc.dataclass
class NVTLangevinState:
    """What ``init_fn`` / ``step_fn`` hand back: the fields the reference reads off jax_md's state (``.position``, ``.mass``:
    mythos/simulators/jax_md/utils.py:19-28, jaxmd.py:84-92) plus the momenta and the step counter.  Self-contained: the
    tensors are copies of the integrator's resident frames, so an older state stays valid and can be stepped again."""

    position: RigidBody
    momentum: RigidBody  # center: linear momenta (N, 3); orientation: body-frame angular momenta (N, 3)
    mass: RigidBody
    step: int
    _version: int = dc.field(default=-1, repr=False)


class NVTLangevin:
    """``init_fn, step_fn = nvt_langevin(energy_fn, shift_fn, dt=, kT=, gamma=)`` - the integrator plug of the reference
    (``simulator_init``, mythos/simulators/jax_md/utils.py:19-28; call sites jaxmd.py:73-92) on the fused HIP kernel.

    ``init_fn(key, R, mass=..., **kw) -> state`` draws the momenta at kT from ``key`` and loads the state into the
    integrator; ``step_fn(state, **kw) -> state`` advances ONE step (the step launch, then a second force launch that closes
    the frame so that it can be read) and reads the frames back, so that every state is a value as it is in JAX: stepping the newest state continues the resident frames, stepping an older one
    reloads it first and reproduces what it produced before to rounding (the noise of a step is a function of key, step and
    nucleotide; a reloaded state's closing half kick and the next opening one are two additions where the resident frames
    have one).  This is the reference's calling shape, at one C-ABI call and four small copies per step; the loop the
    reference builds from it (``run_fn``) is ``HipMDSimulator.run`` - one call for all steps - and that is the fast path.

    ``energy_or_force_fn`` must be one of this package's energy functions (it names the topology, the model and the
    parameters the kernel steps with); an arbitrary Python callable cannot be run by the HIP kernel and is refused.
    ``dtype`` defaults to the reference's fp64; ``neighbors`` as for HipMDSimulator (default: the energy function's pairs).
    """

    def __init__(self, energy_or_force_fn, shift_fn, dt, kT, gamma, dtype=torch.float64, device=None, neighbors=None):  # noqa: N803
        if not isinstance(energy_or_force_fn, EnergyFunction):
            raise NotImplementedError("nvt_langevin steps an energy function of this package (dna1 / dna2 / rna2 / na1); "
                                      f"got {type(energy_or_force_fn).__name__}")
        self.energy_fn, self.shift_fn = energy_or_force_fn, shift_fn
        self.dt, self.kT, self.gamma = float(dt), float(kT), gamma
        self.dtype, self.device, self.neighbors = dtype, device, neighbors
        self._sim = self._integ = None
        self._version = 0

    def __iter__(self):  # init_fn, step_fn = nvt_langevin(...)
        yield self.init_fn
        yield self.step_fn

    def __getitem__(self, k):  # (the marker this function used to return)
        return {"integrator": "nvt_langevin", "dt": self.dt, "kT": self.kT, "gamma": self.gamma}[k]

    def _read(self, mass, step):
        s = self._integ.system
        c, p, ang = (torch.empty((s.n, 3), dtype=s.dtype, device=s.device) for _ in range(3))
        q = torch.empty((s.n, 4), dtype=s.dtype, device=s.device)
        self._integ.store(c, q, p, ang)
        self._version += 1
        return NVTLangevinState(position=RigidBody(center=c, orientation=Quaternion(vec=q)), momentum=RigidBody(center=p, orientation=ang),
                                mass=mass, step=step, _version=self._version)

    def init_fn(self, key, R, mass=None, **_):  # noqa: N803
        if mass is None:
            mass = RigidBody(center=1.0, orientation=(1.0, 1.0, 1.0))
        elif not isinstance(mass, RigidBody):
            m, inertia = mass if isinstance(mass, (tuple, list)) else (mass, (1.0, 1.0, 1.0))
            mass = RigidBody(center=m, orientation=inertia)
        first = self.energy_fn.energy_fns[0] if isinstance(self.energy_fn, ComposedEnergyFunction) else self.energy_fn
        sp = StaticSimulatorParams(seq=first.seq, mass=mass, gamma=self.gamma, bonded_neighbors=first.bonded_neighbors, checkpoint_every=0,
                                   dt=self.dt, kT=self.kT)
        if self._sim is not None:
            self._sim.release()
        self._sim = HipMDSimulator(energy_fn=self.energy_fn, simulator_params=sp, space=(None, self.shift_fn), neighbors=self.neighbors,
                                   save_every=0, dtype=self.dtype, device=self.device)
        system, integ, dev, _, _ = self._sim._prepare(None, int(key), R.center.device)
        self._integ = integ
        c = R.center.to(device=dev, dtype=self.dtype).contiguous().clone()
        q = R.orientation.vec.to(device=dev, dtype=self.dtype).contiguous().clone()
        p, ang = integ.init_momenta()
        integ.load(c, q, p, ang)
        return self._read(mass, 0)

    def step_fn(self, state: NVTLangevinState, **_):
        if self._integ is None:
            raise ValueError("step_fn: call init_fn first")
        integ = self._integ
        if state._version != self._version:  # not the resident frames: make it so
            integ.load(state.position.center.contiguous(), state.position.orientation.vec.contiguous(), state.momentum.center.contiguous(),
                       state.momentum.orientation.contiguous())
            integ.step = int(state.step)
        integ.advance(1)
        return self._read(state.mass, int(state.step) + 1)

    def close(self) -> None:
        if self._sim is not None:
            self._sim.release()
        self._sim = self._integ = None


def nvt_langevin(energy_or_force_fn, shift_fn, dt, kT, gamma, **kw):  # noqa: N803
    """Signature of ``jax_md.simulate.nvt_langevin``.  Called, it returns the (init_fn, step_fn) pair (NVTLangevin);
    passed uncalled as ``simulator_init`` - what the reference's simulators are given - HipMDSimulator recognises it and
    runs the whole loop in one call."""
    return NVTLangevin(energy_or_force_fn, shift_fn, dt, kT, gamma, **kw)


@dc.dataclass(frozen=True, kw_only=True)
class HipMDSimulator(Simulator):
    energy_fn: EnergyFunction
    simulator_params: StaticSimulatorParams
    space: Any = None
    simulator_init: Callable = nvt_langevin
    neighbors: Any = None
    save_every: int = 1
    # The reference computes in fp64 (jax_enable_x64).  The default here is fp32 - north_star's "fp32 forces at 1e-3", with
    # centres carried as hi + lo pairs - because sampling does not need more and runs 1.7x faster;
    # pass dtype=torch.float64 for the reference's precision (the step-by-step oracle tests run there).
    dtype: torch.dtype = torch.float32
    device: Any = None
    trace_energy: bool = False  # energies of the saved steps in trajectory.metadata (the energy-trace instantiation)
    # defaults for callers that only pass parameters (SimpleOptimizer.step: simulator.run(params, **state))
    init_state: Any = None
    n_steps: int | None = None
    key: int = 0
    # Independent replicas of the system advanced by ONE launch per step (free space only): the copies are laid out
    # on a grid far apart and integrated as one system, so 64 replicas of a 64-nt duplex cost a step of a 4 096-nt
    # system, not 64 steps.  Every nucleotide has its own Philox stream, so replicas are statistically independent.
    # The reference runs replicas as separate simulator instances (mythos/simulators/base.py MultiSimulator, Ray).
    n_replicas: int = 1
    # Constant external forces (oxDNA's ``string`` force with ``rate = 0``): ``(index (m,), force (m, 3))`` or the path of an
    # oxDNA external-force file (mythos_amd.input.external_forces).  With replicas the list is repeated per replica at
    # ``index + r * n``.  None: no forces, and exactly the launches of a simulator that never had any.
    external_forces: Any = None
    # Position-dependent forces on centres of mass (mythos_amd.simulators.restraints.Restraints: tethers, sum restraints,
    # group torques - the stretch-torsion protocol), repeated per replica like the constant forces, anchors and targets
    # moved with each replica to its place on the grid; ``anchor=None`` / ``target=None`` resolve from ``init_state``.
    # Combines with ``external_forces``.  None: no restraints, and no launch for them.
    restraints: Any = None
    # oxDNA's point forces (mythos_amd.simulators.restraints.PointForces: moving strings, traps, mutual traps, repulsion
    # planes and spheres) or the path of an oxDNA external-force file (read_external_field), repeated per replica with
    # positions moved to each replica's place.  The moving ones take the integrator's step count, 0 at the start of every
    # run.  A file's constant strings go where ``external_forces`` go, which then has to be None.  Combines with
    # ``external_forces`` and ``restraints``.  None: no point forces, and exactly the launches of a simulator without.
    point_forces: Any = None
    # device-side objects kept between calls: {key: (OxdnaSystem, LangevinIntegrator, ReplicaLayout)}
    _resident: dict = dc.field(default_factory=dict, init=False, repr=False, compare=False)

    def __getstate__(self):  # (the reference's simulators travel through Ray: handles stay behind)
        d = {f.name: getattr(self, f.name) for f in dc.fields(self) if f.name != "_resident"}
        return d

    def __setstate__(self, d):
        for k, v in d.items():
            object.__setattr__(self, k, v)
        object.__setattr__(self, "_resident", {})

    @staticmethod
    def _close_entry(entry) -> None:
        system, integ, _ = entry
        integ.close()
        system.close()

    def release(self) -> None:
        """Free the device-side objects kept from earlier runs."""
        for entry in self._resident.values():
            self._close_entry(entry)
        self._resident.clear()

    def _integrator_constants(self) -> dict:
        sp = self.simulator_params
        mass, inertia = _pair(sp.mass)
        gamma_t, gamma_r = _pair(sp.gamma)
        return {"dt": float(sp.dt), "kT": float(sp.kT), "gamma_t": float(gamma_t), "gamma_r": float(gamma_r),
                "mass": float(np.asarray(mass).reshape(-1)[0]),
                "inertia": tuple(np.asarray(inertia, dtype=np.float64).reshape(-1)[:3].tolist())}

    def _entry_key(self, low, topo, pairs, n_rep, dev) -> tuple:
        """Everything the kept objects are built from, by content."""
        nb = self.neighbors
        nbr_key = ("verlet", float(nb.r_cutoff), float(nb.dr_threshold), int(nb.rebuild_every)) if pairs is None else ("pairs", pair_tag(pairs))
        return (topology_key(low.model, *topo, low.box, self.dtype, dev), n_rep, nbr_key, *self._integrator_constants().values())

    def _entry(self, key_res, low, topo, pairs, layout, dev, seed):
        """The kept (system, integrator) of this key, or a new pair; -> (system, integrator, whether it is new)."""
        entry = self._resident.get(key_res)
        if entry is not None:
            return entry[0], entry[1], False
        seq, is_end, bonded, is_rna = topo
        system = OxdnaSystem(low.model, seq, is_end, bonded, box=low.box, dtype=self.dtype, device=dev, is_rna=is_rna)
        integ = LangevinIntegrator(system, **self._integrator_constants(), seed=int(seed))
        if pairs is None:
            nb = self.neighbors
            integ.set_neighbor_policy(nb.r_cutoff, nb.dr_threshold, nb.rebuild_every)
        else:
            system.set_neighbors(layout.pairs(pairs))
        while len(self._resident) >= 4:  # (a simulator serves one system; a few variants at most)
            self._close_entry(self._resident.pop(next(iter(self._resident))))
        self._resident[key_res] = (system, integ, layout)
        return system, integ, True

    def _external_field(self, n_one):
        """-> (the point forces of this run, its constant forces): the two fields, with a file given as ``point_forces``
        read and its constant strings (``rate = 0``) taken as the constant forces."""
        pf, ext = self.point_forces, self.external_forces
        if isinstance(pf, (str, bytes)) or hasattr(pf, "__fspath__"):
            pf, const = read_external_field(pf, n_one)
            if const[0].size:
                if ext is not None:
                    raise ValueError("point_forces: the file holds constant strings (rate = 0) and external_forces is given as "
                                     "well; put them in one place")
                ext = const
        return pf, ext

    def _apply_point_forces(self, integ, layout, offsets) -> None:
        pf, _ = self._external_field(layout.n_one)
        if not pf:
            if integ.point_forces:
                integ.set_point_forces()
            return
        _, off = layout.restraint_frames(torch.zeros((layout.n_one, 3)), offsets)
        integ.set_point_forces(pf, n_one=layout.n_one, n_rep=layout.n_rep, offsets=off)

    def _apply_external_forces(self, integ, layout, ext) -> None:
        if ext is None:
            if integ.external_forces[0].size:
                integ.set_external_forces()
            return
        if isinstance(ext, (str, bytes)) or hasattr(ext, "__fspath__"):
            ext = read_external_forces(ext, layout.n_one)
        index = np.asarray(ext[0], dtype=np.int64).reshape(-1)
        force = np.asarray(ext[1], dtype=np.float64).reshape(-1, 3)
        if index.size and (index.min() < 0 or index.max() >= layout.n_one):
            raise ValueError(f"external_forces: nucleotide index out of range [0, {layout.n_one})")
        integ.set_external_forces(*layout.forces(index, force))

    def _apply_restraints(self, integ, layout, c_init, offsets) -> None:
        if not self.restraints:
            if integ.restraints:
                integ.set_restraints()
            return
        ref, off = layout.restraint_frames(c_init, offsets)
        integ.set_restraints(self.restraints, ref, n_one=layout.n_one, n_rep=layout.n_rep, offsets=off)

    def _prepare(self, opt_params, key, state_device):
        """The device-side objects of this simulator at ``opt_params``: (system, integrator, device, replicas, nucleotides
        per replica) - built on first use, afterwards the kept ones with the new parameter vector, key and step 0."""
        ef = self.energy_fn.with_params(opt_params) if opt_params else self.energy_fn
        if not isinstance(ef, ComposedEnergyFunction):
            ef = ComposedEnergyFunction(energy_fns=[ef])
        # a term without a temperature of its own is stepped at the thermostat's
        low = lower(ef.energy_fns, ef.weights, kt_default=self.simulator_params.kT)
        dev = torch.device(self.device) if self.device is not None else state_device
        if dev.type != "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        layout = ReplicaLayout(int(self.n_replicas), int(low.seq.shape[0]))
        topo = layout.topology(low.seq, low.is_end, low.bonded, low.is_rna, box=low.box)
        nb = self.neighbors  # an explicit pair list, the energy function's own, or (pairs None) a Verlet list built on the device
        pairs = None if isinstance(nb, VerletNeighborList) else _pairs_2xP(nb.idx if nb is not None else low.unbonded, layout.n_one)
        key_res = self._entry_key(low, topo, pairs, layout.n_rep, dev)
        system, integ, new = self._entry(key_res, low, topo, pairs, layout, dev, key)
        system.set_params(low.flat.detach())  # 2 KB; everything derived from it on the device follows (param_epoch)
        if not new:
            integ.set_seed(int(key))
            integ.step = 0  # a run starts its noise stream at (key, step 0), as a new integrator would
        self._apply_external_forces(integ, layout, self._external_field(layout.n_one)[1])
        # a probabilistic sequence rides along into the dynamics, as it does in the reference - there the stacking /
        # hydrogen-bonding configurations carry pseq into whatever energy function a simulator steps with
        # (dna1/stacking.py:284-285, hydrogen_bonding.py:330-331)
        if low.pseq is not None:
            system.set_pseq(*layout.pseq(*low.pseq))
        elif system._pseq_terms:
            system.set_pseq()
        return system, integ, dev, layout.n_rep, layout.n_one

    def run(self, opt_params: dict, init_state: RigidBody | None = None, n_steps: int | None = None, key: int | None = None,
            **_) -> SimulatorOutput:
        init_state = self.init_state if init_state is None else init_state
        n_steps = self.n_steps if n_steps is None else n_steps
        key = self.key if key is None else key
        if init_state is None or n_steps is None:
            raise ValueError("HipMDSimulator.run needs init_state and n_steps (as arguments or as fields)")
        if self.simulator_init is not nvt_langevin:
            raise NotImplementedError("HipMDSimulator implements nvt_langevin (the integrator every reference example uses)")
        system, integ, dev, n_rep, n_one = self._prepare(opt_params, key, init_state.center.device)
        sp, nb = self.simulator_params, self.neighbors
        c = init_state.center.to(device=dev, dtype=self.dtype).contiguous().clone()
        q = init_state.orientation.vec.to(device=dev, dtype=self.dtype).contiguous().clone()
        r_list = (nb.r_cutoff + nb.dr_threshold) if isinstance(nb, VerletNeighborList) else 4.0
        layout = ReplicaLayout(n_rep, n_one)
        c_init = c
        c, q, offsets = layout.place(c, q, r_list)
        self._apply_restraints(integ, layout, c_init, offsets)
        self._apply_point_forces(integ, layout, offsets)
        p, ang = integ.init_momenta()
        tc, tq, et = integ.run(c, q, p, ang, int(n_steps), save_every=self.save_every, want_energy=self.trace_energy)
        tc, tq, et = layout.unplace_rows(tc, tq, et, offsets)
        c, q = layout.unplace_state(c, q, offsets)
        n_saved = 0 if tc is None else tc.shape[0]
        traj = SimulatorTrajectory(
            center=tc if tc is not None else c[None][:0],
            orientation=Quaternion(vec=tq if tq is not None else q[None][:0]),
            temperature=torch.full((n_saved,), sp.kT, dtype=torch.float64, device=dev),
            metadata=None if et is None else {"energy_terms": et[:, :8], "kinetic": et[:, 8:]},
        )
        final = RigidBody(center=c, orientation=Quaternion(vec=q))
        # the state handed to the next run(params, **state): continue from the last configuration with a new key
        return SimulatorOutput(observables=[traj], state={"init_state": final, "key": int(key) + 1, "final_state": final,
                                                          "momentum": (p, ang), "steps": integ.step})
