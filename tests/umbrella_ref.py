"""Host restatement of the umbrella sampler's boundary (include/mythos_hip.h, mythos_langevin_set_umbrella): the Philox
uniform of (replica, step), the acceptance rule, the chain of held weights, and the lowering of a weights table to the
dense array the kernels index.  Independent of mythos_amd.simulators.umbrella: numpy and the oracle's Philox only."""

from __future__ import annotations

import numpy as np

from oracle.langevin_oracle import philox4x32

STREAM = 4  # streams 0/1 thermostat, 2/3 barostat, 7/8 initial momenta


def uniform(seed: int, replicas, step: int) -> np.ndarray:
    """u of each replica at the boundary whose absolute step count is ``step``: (c[0] + 0.5) 2^-32 of Philox4x32-10 with the
    key (seed lo, seed hi) and the counter {replica, step lo, step hi, 4}."""
    rep = np.asarray(replicas, dtype=np.uint32).reshape(-1)
    ctr = np.zeros((rep.shape[0], 4), dtype=np.uint32)
    ctr[:, 0] = rep
    ctr[:, 1] = step & 0xFFFFFFFF
    ctr[:, 2] = (step >> 32) & 0xFFFFFFFF
    ctr[:, 3] = STREAM
    c = philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return (c[:, 0].astype(np.float64) + 0.5) * 2.0 ** -32


def accepts(u, w_old, w_new) -> np.ndarray:
    """The rule: W(s') > 0 and u W(s) < W(s'), in float64."""
    u, w_old, w_new = (np.asarray(a, dtype=np.float64) for a in (u, w_old, w_new))
    return (w_new > 0.0) & (u * w_old < w_new)


def chain(w_start, w_new, u):
    """Boundaries in order: w_start (n_rep,) the weights held at the start, w_new and u (B, n_rep) -> (accept (B, n_rep)
    bool, w_old (B, n_rep): the weight each replica held when boundary b was decided)."""
    held = np.asarray(w_start, dtype=np.float64).copy()
    acc = np.zeros(np.shape(w_new), dtype=bool)
    old = np.zeros(np.shape(w_new), dtype=np.float64)
    for b in range(acc.shape[0]):
        old[b] = held
        acc[b] = accepts(u[b], held, w_new[b])
        held = np.where(acc[b], w_new[b], held)
    return acc, old


def reachable_shape(ops) -> tuple:
    return tuple((len(o.pairs) if o.kind == "bond" else len(o.interfaces)) + 1 for o in ops)


def dense_table(ops, table) -> np.ndarray:
    """{state tuple (or int): weight} -> the dense row-major array over every reachable state, a missing row 0."""
    dense = np.zeros(reachable_shape(ops), dtype=np.float64)
    for s, w in table.items():
        dense[(int(s),) if np.ndim(s) == 0 else tuple(int(x) for x in s)] = float(w)
    return dense


def accept_probability(w_old: float, w_new: float) -> float:
    """The share of the 2^32 values u = (k + 0.5) 2^-32 the rule accepts: the rule is monotone in u, so the first
    rejected k is found by bisection on ``accepts`` itself."""
    lo, hi = 0, 2 ** 32  # accepts for k < lo ... rejects for k >= hi
    if not accepts((0 + 0.5) * 2.0 ** -32, w_old, w_new):
        return 0.0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if accepts((mid + 0.5) * 2.0 ** -32, w_old, w_new):
            lo = mid
        else:
            hi = mid
    return (lo + 1) / 2.0 ** 32


def stationary(proposal, w) -> np.ndarray:
    """Stationary law, over the states of non-zero weight, of the chain that proposes j from i with probability
    proposal[i, j] and accepts by the rule with u uniform on its 2^32 values.  Solved, not simulated."""
    k = len(w)
    T = np.zeros((k, k))
    for i in range(k):
        if w[i] == 0:
            T[i, i] = 1.0
            continue
        for j in range(k):
            if j != i:
                T[i, j] = proposal[i, j] * accept_probability(w[i], w[j])
        T[i, i] = 1.0 - T[i].sum()
    live = [i for i in range(k) if w[i] > 0]
    A = T[np.ix_(live, live)].T - np.eye(len(live))
    A[-1] = 1.0
    b = np.zeros(len(live))
    b[-1] = 1.0
    out = np.zeros(k)
    out[live] = np.linalg.solve(A, b)
    return out
