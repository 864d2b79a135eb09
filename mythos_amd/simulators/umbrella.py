"""Umbrella sampling on the resident Langevin state, shaped like the reference's ``oxDNAUmbrellaSampler``
(mythos/simulators/oxdna/oxdna.py:225-275): a run under a weights table that returns the trajectory, the order
parameters and weights of its frames (what the reference reads back from oxDNA's energy file,
mythos/simulators/oxdna/utils.py:348-429) and the weights of the next round in ``state["weights"]``.

    sampler = HipUmbrellaSampler(energy_fn=..., simulator_params=..., order_parameters="op.txt", weights=read_weights("wfile.txt"),
                                 segment_steps=50, n_replicas=64, ...)
    out = sampler.run(opt_params, init_state, n_steps, key)
    traj, info = out.observables                      # frames, and their states / weights (UmbrellaInfo)
    tm = MeltingTemp(...)(traj, info.states[:, 0], info.weight, opt_params)
    out = sampler.run(opt_params, **out.state)        # the next round, under state["weights"]

The method is segment-Metropolis on the integrator (include/mythos_hip.h, mythos_langevin_set_umbrella): ``segment_steps``
ordinary steps are a proposal, accepted per replica with the ratio of the weights of the order-parameter states, a
rejected replica going back to its last accepted state with its momenta reversed.  Everything runs on the GPU; the host
sees one stream synchronisation per segment.

Not built: VMMC, order parameters of oxNA systems, and a bias potential on continuous coordinates (the bias is a table
over the discrete states of ``bond`` and ``mindistance`` order parameters, as in the reference's melting workflow).
"""

from __future__ import annotations

import dataclasses as dc
from pathlib import Path
from typing import Any

import numpy as np
import torch

from mythos_amd import _lib
from mythos_amd.energy.base import Quaternion, RigidBody
from mythos_amd.input.order_parameters import KINDS, OrderParameter, read_order_parameters
from mythos_amd.observables.order_parameters import reweight_from_histogram, umbrella_histogram
from mythos_amd.simulators.base import SimulatorOutput
from mythos_amd.simulators.hip_md import HipMDSimulator, nvt_langevin
from mythos_amd.simulators.io import SimulatorTrajectory
from mythos_amd.simulators.neighbors import VerletNeighborList
from mythos_amd.simulators.replicas import ReplicaLayout


def as_order_parameters(order_parameters) -> tuple:
    """A path of an order-parameter file, or a sequence of ``OrderParameter`` -> the tuple."""
    if isinstance(order_parameters, (str, Path)):
        order_parameters = read_order_parameters(order_parameters)
    ops = tuple(order_parameters)
    if not ops or not all(isinstance(o, OrderParameter) for o in ops):
        raise ValueError("order_parameters: a non-empty sequence of OrderParameter, or the path of an order-parameter file")
    return ops


def reachable_shape(ops) -> tuple:
    """States each order parameter can take: pairs + 1 for ``bond``, interfaces + 1 for ``mindistance``."""
    return tuple((len(o.pairs) if o.kind == "bond" else len(o.interfaces)) + 1 for o in ops)


def lower_table(ops, table) -> np.ndarray:
    """A weights table - {state tuple (or int): weight} as ``read_weights`` returns it, or an array with one axis per order
    parameter - as the dense row-major float64 array the kernels index: a missing row is weight 0; an axis holds every
    reachable state (a shorter one is refused, a row outside the reachable states as well)."""
    shape = reachable_shape(ops)
    if isinstance(table, dict):
        dense = np.zeros(shape, dtype=np.float64)
        for s, w in table.items():
            key = (int(s),) if np.ndim(s) == 0 else tuple(int(x) for x in s)
            if len(key) != len(shape) or any(k < 0 or k >= m for k, m in zip(key, shape)):
                raise ValueError(f"the weights table has a row for the state {key}; the order parameters reach {shape}")
            dense[key] = float(w)
        return dense
    dense = np.ascontiguousarray(table, dtype=np.float64)
    if dense.ndim != len(shape) or any(a < m for a, m in zip(dense.shape, shape)):
        raise ValueError(f"a weights table of shape {dense.shape} is too short: the order parameters reach {shape} states "
                         "(a state without weight is given as 0, not left out)")
    return dense


def lower_ops(ops) -> dict:
    """The lists of mythos_umbrella_check / mythos_langevin_set_umbrella (include/mythos_hip.h) of the order parameters."""
    kind = np.ascontiguousarray([KINDS.index(o.kind) for o in ops], dtype=np.int32)
    first = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(o.pairs) for o in ops])]), dtype=np.int32)
    pairs = np.ascontiguousarray([p for o in ops for p in o.pairs], dtype=np.int32).reshape(-1, 2)
    iface_first = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(o.interfaces) for o in ops])]), dtype=np.int32)
    interfaces = np.ascontiguousarray([x for o in ops for x in o.interfaces] or [0.0], dtype=np.float64)
    return {"kind": kind, "first": first, "pairs": pairs, "iface_first": iface_first, "interfaces": interfaces}


def _bias_args(ops, dense):
    a = lower_ops(ops)
    shape = np.ascontiguousarray(dense.shape, dtype=np.int32)
    ip, dp = (lambda x: x.ctypes.data_as(_lib.c_int_p)), (lambda x: x.ctypes.data_as(_lib.c_double_p))
    keep = (a, shape, dense)  # (the pointers below are theirs)
    return keep, (len(ops), ip(a["kind"]), ip(a["first"]), ip(a["pairs"]), int(a["pairs"].shape[0]), ip(a["iface_first"]),
                  dp(a["interfaces"]), ip(shape), dp(dense))


def check_umbrella(n: int, n_rep: int, model: int, bonded, ops, table, segment_steps: int) -> None:
    """The checks of ``LangevinIntegrator.set_umbrella`` without a device (mythos_umbrella_check): raises ValueError with
    the library's message.  ``bonded``: (B, 2) backbone neighbours of one replica; ``table``: dense, as ``lower_table``
    returns it (a dict is lowered first)."""
    ops = as_order_parameters(ops)
    dense = lower_table(ops, table) if isinstance(table, dict) else np.ascontiguousarray(table, dtype=np.float64)
    if dense.ndim != len(ops):
        raise ValueError("a weights table has one axis per order parameter")
    bonded = np.ascontiguousarray(np.asarray(bonded, dtype=np.int32).reshape(-1, 2))
    keep, args = _bias_args(ops, dense)
    _lib.check(_lib.load().mythos_umbrella_check(int(n), int(n_rep), int(model), int(bonded.shape[0]), bonded.ctypes.data_as(_lib.c_int_p),
                                                 *args, int(segment_steps)), "umbrella_check")
    del keep


@dc.dataclass(frozen=True)
class UmbrellaRecord:
    """What every boundary of ``LangevinIntegrator.advance_umbrella`` decided, tensors on the integrator's device with the
    leading shape (n_segments, n_rep): the proposal's order-parameter ``values`` (float64, as ``OxdnaSystem.order_params``
    returns them for the proposal row) and ``states`` (int64), the weight the replica held (``w_old``), the proposal's
    (``w_new``), the uniform ``u``, the decision ``accept`` and the states the replica holds after it (``held``, int64: the
    proposal's where accepted, the ones it held before otherwise - the states of the sample row).  ``prop_center`` /
    ``prop_quat``: the proposals' rows at the sampling boundaries, where asked for."""

    values: torch.Tensor
    states: torch.Tensor
    w_old: torch.Tensor
    w_new: torch.Tensor
    u: torch.Tensor
    accept: torch.Tensor
    held: torch.Tensor
    prop_center: Any = None
    prop_quat: Any = None

    @property
    def w_held(self) -> torch.Tensor:
        """The weight of the state each replica holds after the decision."""
        return torch.where(self.accept, self.w_new, self.w_old)


def record_of(raw: torch.Tensor, n_ops: int, prop_center=None, prop_quat=None) -> UmbrellaRecord:
    """The (n_segments, n_rep, 3 n_ops + 4) rows of mythos_langevin_advance_umbrella as an ``UmbrellaRecord``."""
    return UmbrellaRecord(values=raw[..., :n_ops], states=raw[..., n_ops:2 * n_ops].round().to(torch.int64), w_old=raw[..., 2 * n_ops],
                          w_new=raw[..., 2 * n_ops + 1], u=raw[..., 2 * n_ops + 2], accept=raw[..., 2 * n_ops + 3] > 0.5,
                          held=raw[..., 2 * n_ops + 4:].round().to(torch.int64), prop_center=prop_center, prop_quat=prop_quat)


@dc.dataclass(frozen=True)
class UmbrellaInfo:
    """The order-parameter columns of a sampled trajectory, row for row: ``states`` (F, n_ops) int64, ``weight`` (F,)
    float64 - the umbrella weight of each frame's state - and the order parameters' ``names``.  On the GPU, replica-major
    like the trajectory.  ``MeltingTemp`` takes ``states[:, 0]`` (the ``bond`` column of the usual file) and ``weight``."""

    states: torch.Tensor
    weight: torch.Tensor
    names: tuple


@dc.dataclass(frozen=True, kw_only=True)
class HipUmbrellaSampler(HipMDSimulator):
    """``HipMDSimulator`` under an umbrella bias.  ``order_parameters``: the path of an order-parameter file or
    ``OrderParameter``s (``bond`` / ``mindistance``, nucleotides of one replica); ``weights``: the table - a dict as
    ``read_weights`` returns it, or an array with one axis per order parameter; ``segment_steps``: steps per proposal;
    ``sample_every``: boundaries per saved frame.  ``run(opt_params, init_state, n_steps, key, weights=None)`` takes
    ``n_steps // segment_steps`` segments; ``weights`` replaces the table for this run (the reference's sampler is handed the
    next round's table the same way).  ``observables = [trajectory, UmbrellaInfo]``; ``state`` carries ``weights`` - the
    next round's table, ``reweight_from_histogram(umbrella_histogram(states, weight))`` - and ``acceptance``.  Replicas,
    restraints, point forces and external forces are the parent's; ``save_every`` and ``trace_energy`` are not used."""

    order_parameters: Any = None
    weights: Any = None
    segment_steps: int = 50
    sample_every: int = 1
    hb_cutoff: float = -0.1

    def run(self, opt_params: dict, init_state: RigidBody | None = None, n_steps: int | None = None, key: int | None = None,
            weights=None, **_) -> SimulatorOutput:
        init_state = self.init_state if init_state is None else init_state
        n_steps = self.n_steps if n_steps is None else n_steps
        key = self.key if key is None else key
        table = self.weights if weights is None else weights
        if init_state is None or n_steps is None:
            raise ValueError("HipUmbrellaSampler.run needs init_state and n_steps (as arguments or as fields)")
        if self.order_parameters is None or table is None:
            raise ValueError("HipUmbrellaSampler needs order_parameters and weights")
        if self.simulator_init is not nvt_langevin:
            raise NotImplementedError("HipUmbrellaSampler implements nvt_langevin (the integrator every reference example uses)")
        if self.segment_steps < 1 or self.sample_every < 1:
            raise ValueError("segment_steps and sample_every are at least 1")
        ops = as_order_parameters(self.order_parameters)
        dense = lower_table(ops, table)
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
        integ.set_umbrella(ops, dense, self.segment_steps, n_rep=n_rep, hb_cutoff=self.hb_cutoff)
        integ.load(c, q, p, ang)
        n_seg = int(n_steps) // int(self.segment_steps)
        tc, tq, rec = integ.advance_umbrella(n_seg, sample_every=self.sample_every)
        integ.store(c, q, p, ang)
        accepted, decided = integ.umbrella_counts()
        n_saved = n_seg // self.sample_every
        if n_saved == 0:
            tc, tq = c[None][:0], q[None][:0]
        tc, tq, _ = layout.unplace_rows(tc, tq, None, offsets)
        c, q = layout.unplace_state(c, q, offsets)
        traj = SimulatorTrajectory(center=tc, orientation=Quaternion(vec=tq),
                                   temperature=torch.full((tc.shape[0],), sp.kT, dtype=torch.float64, device=dev), metadata=None)
        # the states and weights the replicas held at the sampling boundaries, as the kernel decided on them: (S, n_rep, .)
        # -> replica-major like the trajectory
        at = slice(self.sample_every - 1, n_saved * self.sample_every, self.sample_every)
        info = UmbrellaInfo(states=rec.held[at].transpose(0, 1).reshape(-1, len(ops)).contiguous(),
                            weight=rec.w_held[at].transpose(0, 1).reshape(-1).contiguous(), names=tuple(o.name for o in ops))
        nxt = reweight_from_histogram(umbrella_histogram(info.states, info.weight, shape=dense.shape)) if n_saved else dense
        final = RigidBody(center=c, orientation=Quaternion(vec=q))
        return SimulatorOutput(observables=[traj, info],
                               state={"init_state": final, "key": int(key) + 1, "final_state": final, "momentum": (p, ang),
                                      "steps": integ.step, "weights": nxt, "acceptance": accepted / max(decided, 1)})
