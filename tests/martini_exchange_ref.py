"""Host restatement of temperature replica exchange in the MARTINI ensemble (include/mythos_hip.h,
mythos_martini_langevin_set_exchange): the pair schedule, the Philox uniform of (rung, step), U, d, the acceptance rule and
the velocity factor in numpy, from ``oracle.langevin_oracle.philox4x32`` alone - and ``OracleChain``, R CPU oracles stepped
from event to event whose kT is swapped and whose velocities are rescaled either by the rule or by decisions handed in.
Independent of mythos_amd."""

from __future__ import annotations

import numpy as np
import torch

from oracle.langevin_oracle import normals6, philox4x32
from oracle.martini_langevin_oracle import MartiniLangevinOracle

STREAM = 5  # streams 0/1 thermostat, 2/3 barostat, 4 umbrella, 7/8 initial velocities
BAR = 16.6053907  # kJ/mol/nm^3 -> bar


def schedule(n_rep: int, attempt: int) -> list[int]:
    """The lower rungs t of the pairs (t, t + 1) that attempt ``attempt`` tries."""
    return list(range(attempt % 2, n_rep - 1, 2))


def uniform(seed: int, rung: int, step: int) -> float:
    """(c[0] + 0.5) 2^-32 of Philox4x32-10 with the key (seed lo, seed hi) and the counter {rung, step lo, step hi, 5}."""
    ctr = np.array([[rung, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, STREAM]], dtype=np.uint32)
    c = philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return float((np.float64(c[0, 0]) + 0.5) * 2.0 ** -32)


def potential(e_row) -> np.float64:
    """U of an energy row (lj, bond, angle, kinetic[, coulomb]): lj + bond + angle (+ coulomb), added in that order."""
    e = np.asarray(e_row, dtype=np.float64)
    u = e[0] + e[1]
    u = u + e[2]
    if e.shape[0] > 4:
        u = u + e[4]
    return u


def volume(box) -> np.float64:
    b = np.asarray(box, dtype=np.float64)
    return (b[0] * b[1]) * b[2]


def delta(kT_t, kT_t1, u_a, v_a, u_b, v_b, p=0.0) -> np.float64:
    """d = (beta_t - beta_t+1) (H_A - H_B), H = U + p V, slot A on rung t and slot B on rung t + 1; float64."""
    f = np.float64
    h_a, h_b = f(u_a) + f(p) * f(v_a), f(u_b) + f(p) * f(v_b)
    return (f(1.0) / f(kT_t) - f(1.0) / f(kT_t1)) * (h_a - h_b)


def accepts(d, u) -> bool:
    return bool(d >= 0.0 or u < np.exp(np.float64(d)))


def factor(kT_old, kT_new, dtype=np.float64):
    """What a slot's velocities are multiplied by: sqrt(kT_new / kT_old) in double, rounded once to ``dtype``."""
    return dtype(np.sqrt(np.float64(kT_new) / np.float64(kT_old)))


def pressure_term(baro) -> float:
    """p of H = U + p V (kJ/mol/nm^3) under the barostat settings ``baro`` (a dict as for set_barostat, or None)."""
    if not baro:
        return 0.0
    ref = np.broadcast_to(np.asarray(baro.get("ref_p", 1.0), dtype=np.float64), (2,))
    beta = np.broadcast_to(np.asarray(baro.get("compressibility", 4.5e-5), dtype=np.float64), (2,))
    if baro.get("coupling", "isotropic") == "isotropic" or beta[0] > 0:
        return float(ref[0] / BAR)
    return float(ref[1] / BAR)


def decide(ladder, kTs, e_rows, boxes, step: int, every: int, seed: int, p: float = 0.0, forced=None):
    """One event at absolute step ``step``: ladder (R,) rung_of_slot, kTs (R,) the rungs' kT, e_rows (R, 4 | 5), boxes (R, 3)
    -> (new ladder, records [dict], factors (R,) float64 - 1.0 where a slot keeps its rung).  ``forced``: {(step, t): bool}
    taken in place of the rule's outcome (d and u are still recorded)."""
    ladder = np.asarray(ladder, dtype=np.int64)
    new, fac, recs = ladder.copy(), np.ones(len(ladder), dtype=np.float64), []
    for t in schedule(len(ladder), step // every):
        a, b = int(np.nonzero(ladder == t)[0][0]), int(np.nonzero(ladder == t + 1)[0][0])
        u_a, u_b, v_a, v_b = potential(e_rows[a]), potential(e_rows[b]), volume(boxes[a]), volume(boxes[b])
        d, u = delta(kTs[t], kTs[t + 1], u_a, v_a, u_b, v_b, p), uniform(seed, t, step)
        acc = accepts(d, u) if forced is None else bool(forced[(step, t)])
        if acc:
            new[a], new[b] = t + 1, t
            fac[a], fac[b] = factor(kTs[t], kTs[t + 1]), factor(kTs[t + 1], kTs[t])
        recs.append(dict(step=step, rung=t, slot_a=a, slot_b=b, u_a=u_a, u_b=u_b, v_a=v_a, v_b=v_b, d=d, u=u, accepted=acc))
    return new, recs, fac


def host_init_velocities(kT: float, seed: int, mass) -> np.ndarray:
    """mm_init_velocities_kernel in float64: sqrt(kT / m) normals6(seed, i, 2^64 - 1, stream 7)[:3], the centre-of-mass
    velocity removed.  Equal to the device's to round-off."""
    m = np.asarray(mass, dtype=np.float64).reshape(-1, 1)
    v = np.sqrt(kT / m) * normals6(seed, m.shape[0], 0xFFFFFFFFFFFFFFFF, stream=7)[:, :3]
    return v - (m * v).sum(0) / m.sum()


class OracleChain:
    """R ``MartiniLangevinOracle``s - the slots - stepped from event to event.  ``baro``: settings as for set_barostat;
    coupling events then follow the exchange of their step (tests/martini_npt_ref.py's event on the slot's own box and kT).
    ``forced``: the decisions {(step, t): bool} to take in place of the rule's."""

    def __init__(self, ff_args, use_g96, boxes, dt, kTs, gamma, mass, seeds, every, seed, baro=None, forced=None):
        self.kTs = np.asarray(kTs, dtype=np.float64)
        self.slots = [MartiniLangevinOracle(*ff_args, use_g96, np.array(box, dtype=np.float64), dt, float(kT), gamma, mass, seed=int(s))
                      for box, kT, s in zip(boxes, self.kTs, seeds)]
        self.ff_args, self.use_g96, self.mass, self.dt = ff_args, use_g96, np.asarray(mass, dtype=np.float64), dt
        self.every, self.seed, self.baro, self.forced = int(every), int(seed), baro, forced
        self.ladder = np.arange(len(self.slots), dtype=np.int64)
        self.log = []
        self.p = pressure_term(baro)

    @property
    def boxes(self):
        return np.stack([o.box.numpy().copy() for o in self.slots])

    def _couple(self, o, x, v):
        from tests import martini_npt_ref as NR

        b = self.baro
        every = int(b["every"])
        ref_p = np.broadcast_to(np.asarray(b["ref_p"], dtype=np.float64), (2,))
        f = np.broadcast_to(np.asarray(b["compressibility"], dtype=np.float64), (2,)) * every * self.dt / b["tau_p"]
        box = o.box.numpy()
        w = NR.strain_virial(x, box, *self.ff_args, self.use_g96)
        P = (NR.kinetic_diag(self.mass, v) + w) / box.prod() * BAR
        xi = normals6(o.seed, 1, o.step_index, stream=2)[0, :2]
        mu = np.exp(NR.log_mu(P, box.prod(), o.kT, b["kind"], b["coupling"], ref_p, f, xi))
        x *= mu
        if b["kind"] == "c-rescale":
            v /= mu
        o.box = o.box * torch.as_tensor(mu)

    def run(self, x, v, n_steps: int, save_every: int = 0):
        """x, v (R, n, 3) float64, in place -> {absolute step: (positions, boxes, energy rows (R, 4), ladder)} of the saved
        rows, each the state before the events of its step."""
        out, done = {}, 0
        c_every = int(self.baro["every"]) if self.baro else 0
        while done < n_steps:
            s = self.slots[0].step_index
            to_x = self.every - s % self.every
            to_c = c_every - s % c_every if c_every else n_steps + 1
            to_save = save_every - done % save_every if save_every > 0 else n_steps + 1
            n = min(to_x, to_c, to_save, n_steps - done)
            e = np.stack([o.run(x[r], v[r], n)[-1] for r, o in enumerate(self.slots)])
            done, s = done + n, s + n
            if n == to_save:
                out[s] = (x.copy(), self.boxes, e.copy(), self.ladder.copy())
            if n == to_x:
                self.ladder, recs, fac = decide(self.ladder, self.kTs, e, self.boxes, s, self.every, self.seed, self.p, self.forced)
                self.log += recs
                for r, o in enumerate(self.slots):
                    v[r] *= fac[r]
                    o.kT = float(self.kTs[self.ladder[r]])
            if n == to_c:
                for r, o in enumerate(self.slots):
                    self._couple(o, x[r], v[r])
        return out
