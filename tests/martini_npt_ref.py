"""CPU references for the MARTINI pressure kernel and barostat (tests/test_gpu_martini_npt.py), built from oracle/.

``strain_virial``   W_d = -dU/ds_d of the oracle's energies at pos * s, box * s (autograd through the minimum image).
``log_mu``          the coupling formulas of include/mythos_hip.h (mythos_martini_langevin_set_barostat), in NumPy.
``NptOracle``       oracle.martini_langevin_oracle.MartiniLangevinOracle stepped from event to event.
``ideal_gas_volumes``  the barostat alone on thermostatted free particles: the statistics of its noise term.
Pinned by tests/test_martini_npt_cpu.py.
"""

from __future__ import annotations

import numpy as np
import torch

from oracle import martini_oracle as mo
from oracle.langevin_oracle import normals6
from oracle.martini_langevin_oracle import MartiniLangevinOracle

BAR = 16.6053907  # kJ/mol/nm^3 -> bar


def _t(a):
    return a.detach().clone().double() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))


def strain_energy(s, pos, box, types, sigma, eps, bonds, bond_k, bond_r0, angles, angle_k, angle_t0, use_g96):
    """U(pos * s, box * s): the affine map of beads and box together, s (3,)."""
    x, b = pos * s, box * s
    bonds, angles = np.asarray(bonds).reshape(-1, 2), np.asarray(angles).reshape(-1, 3)
    u = mo.lj_energy(x, b, types, sigma, eps, bonds)
    if bonds.shape[0]:
        u = u + mo.bond_energy(x, b, bonds, bond_k, bond_r0)
    if angles.shape[0]:
        u = u + mo.angle_energy(x, b, angles, angle_k, angle_t0, use_g96)
    return u


def strain_virial(pos, box, types, sigma, eps, bonds, bond_k, bond_r0, angles, angle_k, angle_t0, use_g96):
    """W (3,) float64 in kJ/mol: -dU/ds at s = 1 (= -dU/dln s)."""
    args = (_t(pos), _t(box), types, _t(sigma), _t(eps), bonds, _t(bond_k), _t(bond_r0), angles, _t(angle_k), _t(angle_t0), use_g96)
    s = torch.ones(3, dtype=torch.float64, requires_grad=True)
    u = strain_energy(s, *args)
    if not u.requires_grad:  # (no pair inside the cut-off, no bond, no angle)
        return np.zeros(3)
    (g,) = torch.autograd.grad(u, s)
    return -g.numpy()


def strain_virial_fd(pos, box, *rest, h=1e-6):
    """The same by central differences in s, one axis at a time."""
    args = (_t(pos), _t(box), rest[0], _t(rest[1]), _t(rest[2]), rest[3], _t(rest[4]), _t(rest[5]), rest[6], _t(rest[7]), _t(rest[8]), rest[9])
    w = np.zeros(3)
    for d in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[d] = h
        w[d] = -(float(strain_energy(1.0 + e, *args)) - float(strain_energy(1.0 - e, *args))) / (2.0 * h)
    return w


def kinetic_diag(mass, v):
    """K (3,) = sum_i m_i v_id^2 in kJ/mol."""
    return (np.asarray(mass, dtype=np.float64).reshape(-1, 1) * np.asarray(v, dtype=np.float64) ** 2).sum(0)


def log_mu(P, V, kT, kind, coupling, ref_p, f, xi):
    """ln mu (3,) of one coupling event.  P (3,) bar, V nm^3, kT kJ/mol, f = beta * every * dt / tau_p (2,) per bar,
    ref_p (2,) bar, xi (2,) standard normals; kind "berendsen" drops the noise terms."""
    kTp = BAR * kT
    noise = 1.0 if kind == "c-rescale" else 0.0
    if coupling == "isotropic":
        p = (P[0] + P[1] + P[2]) / 3.0
        l = (-f[0] * (ref_p[0] - p) + noise * np.sqrt(2.0 * kTp * f[0] / V) * xi[0]) / 3.0
        return np.array([l, l, l])
    pxy = 0.5 * (P[0] + P[1])
    lxy = -f[0] * (ref_p[0] - pxy) / 3.0 + noise * np.sqrt(kTp * f[0] / (3.0 * V)) * xi[0]
    lz = -f[1] * (ref_p[1] - P[2]) / 3.0 + noise * np.sqrt(2.0 * kTp * f[1] / (3.0 * V)) * xi[1]
    return np.array([lxy, lxy, lz])


class NptOracle:
    """MartiniLangevinOracle plus coupling events at every absolute step s > 0 with s % every == 0, on the closed state
    (x_s, v_s) with the box from before the event; xi = normals6(seed, 1, s, stream=2)[0, :2]."""

    def __init__(self, ff_args, use_g96, box, dt, kT, gamma, mass, seed, kind, coupling, ref_p, compressibility, tau_p, every):
        self.ff_args, self.use_g96 = ff_args, use_g96
        self.orc = MartiniLangevinOracle(*ff_args, use_g96, box, dt, kT, gamma, mass, seed=seed)
        self.kind, self.coupling, self.every = kind, coupling, int(every)
        self.ref_p = np.broadcast_to(np.asarray(ref_p, dtype=np.float64), (2,))
        self.f = np.broadcast_to(np.asarray(compressibility, dtype=np.float64), (2,)) * every * dt / tau_p
        self.mass, self.kT, self.seed = np.asarray(mass, dtype=np.float64), kT, seed
        self.events = []  # (step, P (3,), mu (3,))

    @property
    def box(self):
        return self.orc.box.numpy().copy()

    def pressure(self, x, v):
        box = self.orc.box.numpy()
        w = strain_virial(x, box, *self.ff_args, self.use_g96)
        k = kinetic_diag(self.mass, v)
        return k, w, (k + w) / box.prod() * BAR

    def run(self, x, v, n_steps, save_every=0):
        """In place; -> (rows (S, n, 3), boxes (S, 3)): row r is the state after (r + 1) * save_every steps of this call,
        before the event of that step if there is one."""
        rows, boxes, done = [], [], 0
        while done < n_steps:
            s = self.orc.step_index
            to_event = self.every - s % self.every
            to_save = save_every - done % save_every if save_every > 0 else n_steps + 1
            n = min(to_event, to_save, n_steps - done)
            self.orc.run(x, v, n)
            done += n
            if n == to_save:
                rows.append(x.copy()), boxes.append(self.box)
            if n == to_event:
                _, _, P = self.pressure(x, v)
                xi = normals6(self.seed, 1, self.orc.step_index, stream=2)[0, :2]
                mu = np.exp(log_mu(P, self.orc.box.numpy().prod(), self.kT, self.kind, self.coupling, self.ref_p, self.f, xi))
                x *= mu
                if self.kind == "c-rescale":
                    v /= mu
                self.orc.box = self.orc.box * torch.as_tensor(mu)
                self.events.append((self.orc.step_index, P, mu))
        return np.array(rows), np.array(boxes)


def ideal_gas_volumes(coupling, beta_z_on, n_steps, *, n=64, kT=2.27, mass=72.0, gamma=1.0, dt=0.02, edge=4.0, f_p0=0.05, seed=0):
    """V after every step of n free particles under the Langevin thermostat (the O step of BAOAB; without forces the
    kicks do nothing and the positions do not enter the pressure) and a c-rescale event after every step, with
    P0 = n kT / edge^3 and f P0 = ``f_p0``.  -> (V (n_steps,), P0 in kJ/mol/nm^3)."""
    rng = np.random.default_rng(seed)
    p0 = n * kT / edge**3  # kJ/mol/nm^3
    ref_p = np.array([p0, p0]) * BAR
    f = np.array([f_p0 / (p0 * BAR), (f_p0 / (p0 * BAR)) if beta_z_on else 0.0])
    c1 = np.exp(-gamma * dt)
    c2 = np.sqrt(kT * (1.0 - c1 * c1) / mass)
    v = np.sqrt(kT / mass) * rng.standard_normal((n, 3))
    box = np.full(3, edge)
    out = np.empty(n_steps)
    for s in range(n_steps):
        v = c1 * v + c2 * rng.standard_normal((n, 3))
        V = box.prod()
        P = mass * (v * v).sum(0) / V * BAR
        mu = np.exp(log_mu(P, V, kT, "c-rescale", coupling, ref_p, f, rng.standard_normal(2)))
        box = box * mu
        v = v / mu
        out[s] = box.prod()
    return out, p0


def volume_statistics(V, n, kT, p0, blocks=50):
    """After dropping the first tenth: (z = (<V> - (n + 1) kT / P0) / SE with SE from ``blocks`` block means,
    Var V / <V>^2 * (n + 1))."""
    V = np.asarray(V)[len(V) // 10:]
    m = V.mean()
    bm = V[: len(V) // blocks * blocks].reshape(blocks, -1).mean(1)
    se = bm.std(ddof=1) / np.sqrt(blocks)
    return (m - (n + 1) * kT / p0) / se, V.var() / m**2 * (n + 1)
