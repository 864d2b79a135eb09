"""oxDNA's ``bond`` and ``mindistance`` order parameters of stored frames, and the umbrella-sampling bookkeeping built
on them: the states and weights ``MeltingTemp`` takes, the per-state histogram oxDNA writes as ``last_hist.dat`` and
the weights the reference derives from it (mythos/simulators/oxdna/oxdna.py:213-221, utils.py:348-429).

The definitions (checked against oxDNA's own columns of tests/golden/melting_temp on every frame):

``bond``: the number of listed pairs whose hydrogen-bonding energy is below ``hb_cutoff`` (oxDNA's ``HB_CUTOFF``,
-0.1; strictly below).  The energy is the one the energy kernel sums, under the energy function's current parameters and
sequence weights.  ``mindistance``: the smallest minimum-image distance between the base (hydrogen-bonding) sites of
the listed pairs; its state is the number of ``interfaces`` the distance exceeds (strictly).

Evaluated by one launch of mythos_oxdna_order_params per call, one lane per (frame, pair).  The sampling run that
produces such frames is mythos_amd.simulators.umbrella.HipUmbrellaSampler.  Not built: VMMC, order parameters inside the
energy or MD step launches, oxNA, gradients, and an all-pairs hydrogen-bond count over the neighbour rows.
"""

from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from mythos_amd.input.order_parameters import OrderParameter, read_order_parameters


class OrderParameters:
    """The order parameters of an oxDNA order-parameter file, evaluated on trajectories under ``energy_fn``.

    ``order_parameters``: a sequence of ``OrderParameter``, or the path of an order-parameter file.  ``energy_fn``: a
    ``ComposedEnergyFunction`` of oxDNA1, oxDNA2 or oxRNA2 with a discrete sequence; its topology decides which pairs
    may be listed - oxDNA evaluates no hydrogen bond between backbone neighbours, so such a pair is refused.

    ``op(trajectory, opt_params=None)``: the (F, n_ops) int64 states on the trajectory's device - the count for
    ``bond``, the interface index for ``mindistance``.  Column 0 of a file whose first block is the ``bond`` parameter
    is the ``bind_states`` of ``MeltingTemp``.  The states are integers and carry no gradient: a frame's state is
    piecewise constant in the parameters, and the melting temperature is differentiated through the energies alone, as
    in the reference."""

    def __init__(self, order_parameters, energy_fn, hb_cutoff: float = -0.1):
        if isinstance(order_parameters, (str, Path)):
            order_parameters = read_order_parameters(order_parameters)
        self.ops = tuple(order_parameters)
        if not self.ops or not all(isinstance(o, OrderParameter) for o in self.ops):
            raise ValueError("order_parameters: a non-empty sequence of OrderParameter, or the path of an order-parameter file")
        self.energy_fn = energy_fn
        self.hb_cutoff = float(hb_cutoff)
        first = energy_fn.energy_fns[0]
        n = int(np.asarray(first.seq).shape[0])
        bonded = np.asarray(first.bonded_neighbors.detach().cpu() if isinstance(first.bonded_neighbors, torch.Tensor) else first.bonded_neighbors)
        bonds = {(min(int(i), int(j)), max(int(i), int(j))) for i, j in bonded.reshape(-1, 2)}
        for o in self.ops:
            for i, j in o.pairs:
                if i >= n or j >= n:
                    raise ValueError(f"order parameter '{o.name}' names nucleotide {max(i, j)}; the topology has {n}")
                if (min(i, j), max(i, j)) in bonds:
                    raise ValueError(f"order parameter '{o.name}' lists the pair ({i}, {j}), backbone neighbours in the topology: "
                                     "oxDNA evaluates no hydrogen bond between them")

    @property
    def names(self) -> tuple:
        return tuple(o.name for o in self.ops)

    def values(self, trajectory, opt_params=None, *, raw: bool = False):
        """The (F, n_ops) float64 rows: the bond count and the smallest distance, before the interfaces.  ``raw``: also the
        (F, P) hydrogen-bonding energies and base-base distances of the listed pairs (``OxdnaSystem.order_params``)."""
        from mythos_amd.energy.base import _apply_pseq, _get_system, _set_flat
        from mythos_amd.energy.lowering import lower

        fn = self.energy_fn if opt_params is None else self.energy_fn.with_params(opt_params)
        low = lower(fn.energy_fns, fn.weights)
        if low.pseq is not None:
            raise ValueError("the energy function carries a probabilistic sequence: an expected hydrogen-bonding energy below "
                             "the cutoff is not oxDNA's order parameter")
        center, quat = trajectory.center, trajectory.orientation.vec
        if center.dim() != 3:
            raise ValueError("order parameters take a trajectory: center (n_states, N, 3)")
        entry = _get_system(low, center.dtype, center.device)
        _apply_pseq(entry, None)
        system = _set_flat(entry, low.flat)
        return system.order_params(center.detach(), quat.detach(), self.ops, raw=raw, hb_cutoff=self.hb_cutoff)

    def states_of(self, values: torch.Tensor) -> torch.Tensor:
        """(F, n_ops) int64 states of the float rows ``values``."""
        cols = []
        for k, o in enumerate(self.ops):
            v = values[:, k]
            if o.kind == "bond":
                cols.append(v.round().to(torch.int64))
            else:
                iface = torch.as_tensor(o.interfaces, dtype=v.dtype, device=v.device)
                cols.append((v[:, None] > iface[None, :]).sum(1).to(torch.int64))
        return torch.stack(cols, dim=1)

    def __call__(self, trajectory, opt_params=None) -> torch.Tensor:
        return self.states_of(self.values(trajectory, opt_params))

    def weights(self, states, table) -> torch.Tensor:
        """(F,) float64 umbrella weights of the (F, n_ops) ``states`` looked up in ``table`` - {state tuple: weight}
        (``read_weights``) or an array with one axis per order parameter.  A state without a row is an error."""
        dev = states.device if isinstance(states, torch.Tensor) else None
        st = np.asarray(states.detach().cpu() if isinstance(states, torch.Tensor) else states, dtype=np.int64).reshape(-1, len(self.ops))
        if isinstance(table, dict):
            rows = {((int(s),) if np.ndim(s) == 0 else tuple(int(x) for x in s)): float(w) for s, w in table.items()}
            uniq, inverse = np.unique(st, axis=0, return_inverse=True)
            missing = [tuple(int(x) for x in u) for u in uniq if tuple(int(x) for x in u) not in rows]
            if missing:
                raise KeyError(f"the weights table has no row for the state(s) {missing}")
            w = np.asarray([rows[tuple(int(x) for x in u)] for u in uniq], dtype=np.float64)[inverse.reshape(-1)]
        else:
            arr = np.asarray(table, dtype=np.float64)
            if arr.ndim != len(self.ops) or (st < 0).any() or (st >= np.asarray(arr.shape)[None, :]).any():
                raise KeyError("the weights table has no row for some of the states")
            w = arr[tuple(st.T)]
        return torch.as_tensor(w, dtype=torch.float64, device=dev)


def _states_2d(states) -> np.ndarray:
    st = np.asarray(states.detach().cpu() if isinstance(states, torch.Tensor) else states, dtype=np.int64)
    return st.reshape(-1, 1) if st.ndim == 1 else st


def _shape_of(st: np.ndarray, shape) -> tuple:
    if (st < 0).any():
        raise ValueError("states are non-negative")
    full = tuple(int(m) + 1 for m in st.max(0)) if shape is None else tuple(int(x) for x in np.atleast_1d(shape))
    if len(full) != st.shape[1] or (st >= np.asarray(full)[None, :]).any():
        raise ValueError(f"shape {full} does not hold the states")
    return full


def umbrella_histogram(states, weights, shape=None) -> dict:
    """The first columns of oxDNA's ``last_hist.dat`` from the (F,) or (F, n_ops) ``states`` and the (F,) umbrella
    ``weights`` of a trajectory: {"count": frames per state, "unbiased_count": sum of 1 / weight per state}, float64
    arrays of ``shape`` (default: largest state + 1 along every order parameter)."""
    st = _states_2d(states)
    full = _shape_of(st, shape)
    w = np.asarray(weights.detach().cpu() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != st.shape[0]:
        raise ValueError("one weight per frame")
    flat = np.ravel_multi_index(tuple(st.T), full)
    size = int(np.prod(full))
    return {"count": np.bincount(flat, minlength=size).astype(np.float64).reshape(full),
            "unbiased_count": np.bincount(flat, weights=1.0 / w, minlength=size).reshape(full)}


def extrapolated_histogram(e0, et, kt_sim, kts, states, weights, shape=None) -> torch.Tensor:
    """The unbiased histogram extrapolated to every temperature of ``kts``, (T, *shape): the remaining columns of
    ``last_hist.dat`` up to one factor per temperature.  ``e0`` (F,) energies at the simulation temperature ``kt_sim``,
    ``et`` (T, F) at ``kts``; differentiable in both.  The exponent E_0 / kT_sim - E_t / kT_t is shifted by its largest
    value at each temperature before ``exp``, exactly as ``extrapolated_ratios`` does: summing the bound states and
    dividing by the unbound one gives the ratio in there before the finite-size correction."""
    et = torch.as_tensor(et)
    e0 = torch.as_tensor(e0, device=et.device).to(et)
    kts = torch.as_tensor(np.asarray(kts) if not isinstance(kts, torch.Tensor) else kts, device=et.device).to(et)
    w = torch.as_tensor(np.asarray(weights) if not isinstance(weights, torch.Tensor) else weights, device=et.device).to(et)
    st = _states_2d(states)
    full = _shape_of(st, shape)
    flat = torch.as_tensor(np.ravel_multi_index(tuple(st.T), full), dtype=torch.int64, device=et.device)
    expo = (e0 / kt_sim)[None, :] - et / kts[:, None]
    counts = (1 / w)[None, :] * torch.exp(expo - expo.detach().max(dim=1, keepdim=True).values)
    size = int(np.prod(full))
    hist = torch.zeros((et.shape[0], size), dtype=et.dtype, device=et.device).index_add(1, flat, counts)
    return hist.reshape(et.shape[0], *full)


def reweight_from_histogram(hist) -> np.ndarray:
    """The umbrella weights of the next round from a histogram (``_reweight_from_histogram``, oxdna.py:213-221): 1 /
    unbiased count, divided by the smallest such value, and 0 for a state that was never visited.  ``hist``: the dict of
    ``umbrella_histogram`` or its ``unbiased_count`` array; returns an array of the same shape (``write_weights`` takes it)."""
    unbiased = np.asarray(hist["unbiased_count"] if isinstance(hist, dict) else hist, dtype=np.float64)
    seen = unbiased > 0
    if not seen.any():
        raise ValueError("the histogram is empty")
    w = np.zeros_like(unbiased)
    w[seen] = 1.0 / unbiased[seen]
    return w / w[seen].min()
