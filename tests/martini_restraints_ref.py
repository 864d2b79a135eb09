"""NumPy reference of the MARTINI integrator's external forces - TEST INFRASTRUCTURE ONLY.

The laws of the restraints (position, flat-bottom, pull coordinates between centres of mass) written from their
definition, directly on the dataclasses of mythos_amd.simulators.martini_restraints: nothing here goes through
``MartiniRestraints.lower`` or the library.  Everything is float64; centres of mass are plain mass-weighted sums.

``field(rs, x, masses, box, s, dt, rep, reference_pos)`` -> (F (n, 3), energies (4,) = position, flat-bottom, umbrella,
constant-force, xi (P,)) for replica ``rep`` of the set at step count ``s``.
"""

from __future__ import annotations

import numpy as np

AX = {"x": 0, "y": 1, "z": 2, 0: 0, 1: 1, 2: 2}


def _of_replica(v, rep):
    v = np.asarray(v, dtype=np.float64)
    return float(v) if v.ndim == 0 else float(v[rep])


def group_com(x, masses, members, box=None, pbc_ref=None):
    """Mass-weighted centre of ``members``; with ``pbc_ref`` every member at its minimum image relative to that bead."""
    members = np.asarray(members, dtype=np.int64)
    y = x[members]
    if pbc_ref is not None:
        d = y - x[pbc_ref]
        y = x[pbc_ref] + d - box * np.round(d / box)
    m = masses[members]
    return (m[:, None] * y).sum(0) / m.sum(), m.sum()


def pull(c, x, masses, box, t, rep, topology=None):
    """-> (xi, U, dU/dxi, e = dxi/dX_B (3,), members_a or None, members_b)."""
    mb = c.group_b.indices(topology)
    xb, _ = group_com(x, masses, mb, box, c.group_b.pbc_ref)
    if c.group_a is None:
        ma, xa = None, np.asarray(c.origin, dtype=np.float64)
    else:
        ma = c.group_a.indices(topology)
        xa, _ = group_com(x, masses, ma, box, c.group_a.pbc_ref)
    d = xb - xa
    if c.periodic:
        d = d - box * np.round(d / box)
    if c.geometry == "direction":
        n = np.asarray(c.vec, dtype=np.float64)
        e = n / np.linalg.norm(n)
        xi = float(d @ e)
    else:
        d = d * np.asarray(c.dim, dtype=np.float64)
        xi = float(np.sqrt(d @ d))
        e = d / xi if xi > 0 else np.zeros(3)
    k = _of_replica(c.k, rep)
    if c.kind == "constant-force":
        return xi, k * xi, k, e, ma, mb
    dev = xi - _of_replica(c.init, rep) - c.rate * t
    return xi, 0.5 * k * dev * dev, k * dev, e, ma, mb


def flat_distance(f, x_i, ref):
    rho = x_i - ref
    a = AX[f.axis]
    if f.shape == "cylinder":
        rho[a] = 0.0
    elif f.shape == "layer":
        keep = rho[a]
        rho[:] = 0.0
        rho[a] = keep
    return rho, float(np.sqrt(rho @ rho))


def field(rs, x, masses, box=None, s=0, dt=0.0, rep=0, reference_pos=None, topology=None):
    x = np.asarray(x, dtype=np.float64)
    masses = np.asarray(masses, dtype=np.float64)
    box = None if box is None else np.asarray(box, dtype=np.float64)
    F = np.zeros_like(x)
    e = np.zeros(4)
    t = s * dt

    def ref_of(term):
        return np.asarray(reference_pos[term.index] if term.reference is None else term.reference, dtype=np.float64)

    for p in rs.position:
        k = np.broadcast_to(np.asarray(p.k, dtype=np.float64), (3,))
        d = x[p.index] - ref_of(p)
        e[0] += 0.5 * float((k * d * d).sum())
        F[p.index] -= k * d
    for f in rs.flat_bottom:
        rho, d = flat_distance(f, x[f.index].copy(), ref_of(f))
        active = d < f.r if f.invert else d > f.r
        if active:
            e[1] += 0.5 * f.k * (d - f.r) ** 2
            if d > 0:
                F[f.index] -= f.k * (d - f.r) * rho / d
    xi = np.zeros(len(rs.pulls))
    for j, c in enumerate(rs.pulls):
        xi[j], u, du, ev, ma, mb = pull(c, x, masses, box, t, rep, topology)
        e[3 if c.kind == "constant-force" else 2] += u
        F[mb] -= du * ev[None, :] * (masses[mb] / masses[mb].sum())[:, None]
        if ma is not None:
            F[ma] += du * ev[None, :] * (masses[ma] / masses[ma].sum())[:, None]
    return F, e, xi


def energy(rs, x, masses, box=None, s=0, dt=0.0, rep=0, reference_pos=None):
    return float(field(rs, x, masses, box, s, dt, rep, reference_pos)[1].sum())
