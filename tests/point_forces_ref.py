"""NumPy fp64 reference of the point forces of the oxDNA Langevin integrator (mythos_langevin_set_point_forces): oxDNA's
five laws on single nucleotides and their energies, straight from their definitions, on top of tests/ext_field_ref.py
(the constant forces and the three restraint laws, re-exported here).  ``s`` is the step count of the frame ``x``."""

import numpy as np

from mythos_amd.simulators.restraints import MovingString, MutualTrap, RepulsionPlane, RepulsionSphere, Trap
from tests.ext_field_ref import TORQUE_FLOOR, group_torque, resolved, sum_restraint, tether  # noqa: F401
from tests.ext_field_ref import field as restraint_field

KINDS = (MovingString, Trap, MutualTrap, RepulsionPlane, RepulsionSphere)  # the order of the energy words 3 .. 7


def _unit(d):
    d = np.asarray(d, dtype=np.float64)
    return d / np.linalg.norm(d)


def string(x, t, s, origin=(0.0, 0.0, 0.0)):
    """-> (force (3,) on t.particle, energy)."""
    d, f = _unit(t.dir), t.F0 + t.rate * s
    return f * d, -f * float(d @ (x[t.particle] - np.asarray(origin, dtype=np.float64)))


def trap(x, t, s):
    d = _unit(t.dir) if t.rate != 0 else np.zeros(3)
    dx = x[t.particle] - np.asarray(t.pos0, dtype=np.float64) - t.rate * s * d
    return -t.stiff * dx, 0.5 * t.stiff * float(dx @ dx)


def mutual_trap(x, t, s, box=None):
    D = x[t.ref_particle] - x[t.particle]
    if t.pbc and box is not None:
        L = np.asarray(box, dtype=np.float64)
        D = D - L * np.rint(D / L)
    r = float(np.linalg.norm(D))
    stretch = r - t.r0 - t.rate * s
    return (t.stiff * stretch * D / r if r > 0 else np.zeros(3)), 0.5 * t.stiff * stretch * stretch


def repulsion_plane(x, t, s):
    d = _unit(t.dir)
    h = float(d @ x[t.particle]) + t.position
    return (-t.stiff * h * d, 0.5 * t.stiff * h * h) if h < 0 else (np.zeros(3), 0.0)


def repulsion_sphere(x, t, s):
    rho = x[t.particle] - np.asarray(t.center, dtype=np.float64)
    dist, R = float(np.linalg.norm(rho)), t.r0 + t.rate * s
    if not (dist > R and dist > 0):
        return np.zeros(3), 0.0
    return -t.stiff * (1.0 - R / dist) * rho, 0.5 * t.stiff * (dist - R) ** 2


def point_term(x, t, s, box=None, origin=(0.0, 0.0, 0.0)):
    if isinstance(t, MovingString):
        return string(x, t, s, origin)
    if isinstance(t, MutualTrap):
        return mutual_trap(x, t, s, box)
    return {Trap: trap, RepulsionPlane: repulsion_plane, RepulsionSphere: repulsion_sphere}[type(t)](x, t, s)


def point_field(x, pf, s, box=None, origin=(0.0, 0.0, 0.0)):
    """-> (force (n, 3), energies (5,) by kind) of the point forces ``pf`` alone."""
    x = np.asarray(x, dtype=np.float64)
    F, e = np.zeros_like(x), np.zeros(len(KINDS))
    for t in pf.terms:
        f, u = point_term(x, t, s, box, origin)
        F[t.particle] += f
        e[KINDS.index(type(t))] += u
    return F, e


def field(x, rs, pf, s, const=None, box=None, origin=(0.0, 0.0, 0.0)):
    """The whole external field -> (force (n, 3), energies (8,): the three of ext_field_ref.field, then one per kind)."""
    F, e = restraint_field(x, rs, const)
    Fp, ep = point_field(x, pf, s, box, origin)
    return F + Fp, np.concatenate([e, ep])
