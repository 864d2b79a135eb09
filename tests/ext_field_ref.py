"""NumPy fp64 reference of the external field of the oxDNA Langevin integrator (mythos_langevin_set_restraints): the
three force laws and the two energies, straight from their definitions.  ``rs`` is a
mythos_amd.simulators.restraints.Restraints whose anchors and targets are resolved (not None)."""

import numpy as np

TORQUE_FLOOR = 1e-24  # S <= floor * sum |x_j|^2 counts as zero (include/mythos_hip.h)


def tether(x, index, k, anchor, axes):
    """-> (forces (m, 3) on the listed nucleotides, energy)."""
    d = (x[list(index)] - np.asarray(anchor, dtype=np.float64).reshape(-1, 3)) * np.asarray(axes, dtype=np.float64)
    return -k * d, 0.5 * k * float((d * d).sum())


def sum_restraint(x, index, k, target, axes):
    d = (x[list(index)].sum(axis=0) - np.asarray(target, dtype=np.float64)) * np.asarray(axes, dtype=np.float64)
    return np.tile(-k * d, (len(index), 1)), 0.5 * k * float(d @ d)


def group_torque(x, index, torque):
    xs = x[list(index)]
    T = np.asarray(torque, dtype=np.float64)
    t = T / np.linalg.norm(T)
    d = xs - xs.mean(axis=0)
    perp = d - np.outer(d @ t, t)
    S = float((perp * perp).sum())
    if S <= TORQUE_FLOOR * float((xs * xs).sum()):
        return np.zeros_like(xs)
    return np.cross(T, d) / S


def field(x, rs, const=None):
    """-> (force (n, 3), energies (3,): -sum F.x of the constant forces, tethers, sum restraints)."""
    x = np.asarray(x, dtype=np.float64)
    F = np.zeros_like(x)
    e = np.zeros(3)
    if const is not None and len(const[0]):
        idx, f = np.asarray(const[0]), np.asarray(const[1], dtype=np.float64).reshape(-1, 3)
        np.add.at(F, idx, f)
        e[0] = -float((f * x[idx]).sum())
    for t in rs.tethers:
        f, u = tether(x, t.index, t.k, t.anchor, t.axes)
        np.add.at(F, list(t.index), f)
        e[1] += u
    for s in rs.sums:
        f, u = sum_restraint(x, s.index, s.k, s.target, s.axes)
        np.add.at(F, list(s.index), f)
        e[2] += u
    for q in rs.torques:
        np.add.at(F, list(q.index), group_torque(x, q.index, q.torque))
    return F, e


def resolved(rs, x0):
    """``rs`` with the None anchors / targets taken from the state ``x0`` (n, 3)."""
    import dataclasses as dc

    x0 = np.asarray(x0, dtype=np.float64)
    tethers = [dc.replace(t, anchor=x0[list(t.index)]) if t.anchor is None else t for t in rs.tethers]
    sums = [dc.replace(s, target=x0[list(s.index)].sum(axis=0)) if s.target is None else s for s in rs.sums]
    return dc.replace(rs, tethers=tuple(tethers), sums=tuple(sums))
