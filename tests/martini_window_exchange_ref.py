"""Host restatement of window exchange in the MARTINI ensemble (include/mythos_hip.h,
mythos_martini_langevin_set_window_exchange) - TEST INFRASTRUCTURE ONLY.

Hamiltonian replica exchange between the per-replica parameter rows ("windows") of a set of restraints at one kT.  The
restraint energies come from tests/martini_restraints_ref.py with the parameter row chosen separately from the
configuration; the pair schedule, the acceptance rule and the Philox uniform are those of tests/martini_exchange_ref.py on
stream 6.  Independent of mythos_amd's library."""

from __future__ import annotations

import numpy as np

from oracle.langevin_oracle import philox4x32
from tests import martini_restraints_ref as REF
from tests.martini_exchange_ref import accepts, schedule  # noqa: F401  (the same schedule and the same rule)

STREAM = 6  # 5 is temperature exchange


def uniform(seed: int, rung: int, step: int) -> float:
    """(c[0] + 0.5) 2^-32 of Philox4x32-10 with the key (seed lo, seed hi) and the counter {rung, step lo, step hi, 6}."""
    ctr = np.array([[rung, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, STREAM]], dtype=np.uint32)
    c = philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return float((np.float64(c[0, 0]) + 0.5) * 2.0 ** -32)


def cross_energy(rs, x, masses, box, step, dt, window, reference_pos=None) -> float:
    """E_w(x, t): the four restraint energies of configuration ``x`` in ITS box under the parameters of window ``window`` -
    the per-replica k and init of that replica, the references left None from ``reference_pos[window]`` - at t = step dt."""
    ref = None if reference_pos is None else np.asarray(reference_pos, dtype=np.float64)
    if ref is not None and ref.ndim == 3:
        ref = ref[window]
    return float(REF.field(rs, x, masses, box, step, dt, window, ref)[1].sum())


def delta(kT, e_t_a, e_t1_a, e_t_b, e_t1_b) -> np.float64:
    """d = -(1 / kT) [(E_t+1(x_A) + E_t(x_B)) - (E_t(x_A) + E_t+1(x_B))], slot A in window t and slot B in window t + 1."""
    f = np.float64
    return -(f(1.0) / f(kT)) * ((f(e_t1_a) + f(e_t_b)) - (f(e_t_a) + f(e_t1_b)))


def decide(windows, kT, energy_of, step: int, every: int, seed: int):
    """One event at absolute step ``step``: windows (R,) window_of_slot, ``energy_of(slot, window)`` -> E_window(x_slot)
    -> (new assignment, records [dict])."""
    windows = np.asarray(windows, dtype=np.int64)
    new, recs = windows.copy(), []
    for t in schedule(len(windows), step // every):
        a, b = int(np.nonzero(windows == t)[0][0]), int(np.nonzero(windows == t + 1)[0][0])
        e = [energy_of(a, t), energy_of(a, t + 1), energy_of(b, t), energy_of(b, t + 1)]
        d, u = delta(kT, *e), uniform(seed, t, step)
        acc = accepts(d, u)
        if acc:
            new[a], new[b] = t + 1, t
        recs.append(dict(step=step, rung=t, slot_a=a, slot_b=b, e_t_a=e[0], e_t1_a=e[1], e_t_b=e[2], e_t1_b=e[3], d=d, u=u, accepted=acc))
    return new, recs


def permute_rows(rows, windows):
    """Per-window rows (R, ...) -> per-slot rows under the assignment ``windows``: slot s holds rows[windows[s]]."""
    return np.asarray(rows)[np.asarray(windows, dtype=np.int64)]


def lowered_for(arrays: dict, windows) -> dict:
    """The arrays of ``MartiniRestraints.lower`` with the parameter rows of slot s those of window windows[s]; topology and
    boxes stay the slots'."""
    out = dict(arrays)
    for key in ("pr_ref", "fb_param", "p_param"):
        out[key] = np.ascontiguousarray(permute_rows(arrays[key], windows))
    return out


def round_trips(window_rows) -> np.ndarray:
    """Completed trips rung 0 -> R - 1 -> 0 of every slot, written from the definition: the visits of the two end rungs in
    order, consecutive repeats dropped, counted from the first visit of rung 0 in pairs (top, bottom)."""
    w = np.asarray(window_rows, dtype=np.int64)
    top = w.shape[1] - 1
    out = np.zeros(w.shape[1], dtype=np.int64)
    for s in range(w.shape[1]):
        ends = [int(g) for g in w[:, s] if g in (0, top)]
        ends = [g for k, g in enumerate(ends) if k == 0 or g != ends[k - 1]]
        if 0 in ends and top > 0:
            ends = ends[ends.index(0):]
            out[s] = (len(ends) - 1) // 2
    return out
