"""Reaction-field Coulomb of a MARTINI system, restated in fp64 NumPy: the pin of the Coulomb kernels.

The reference ships no GROMACS Coulomb energies (its goldens are lj.xvg, bond.xvg, angle.xvg), so what the kernels are
held to is the formula of the GROMACS manual for ``coulombtype = reaction-field`` with the Verlet scheme's potential
shift, written here independently of the device code: all pairs, minimum image, one cut-off.

    f = 138.935458,  k_rf = (eps_rf - eps_r) / ((2 eps_rf + eps_r) r_c^3)  (eps_rf = 0: infinity, 1 / (2 r_c^3)),
    c_rf = 1 / r_c + k_rf r_c^2
    non-excluded pair, r < r_c:   V = (f / eps_r) q_i q_j (1 / r + k_rf r^2 - c_rf)
    excluded (bonded) pair, r < r_c:  V = (f / eps_r) q_i q_j (k_rf r^2 - c_rf)
    self term:                    -1/2 (f / eps_r) c_rf sum q_i^2
    virial per axis:              W_d = -sum_pairs (dV/dr) d_d^2 / r

Units: nm, kJ/mol, e.
"""

from __future__ import annotations

import numpy as np

F_ELEC = 138.935458
PARTS = ("pair", "excluded", "self")


def constants(r_cut: float, epsilon_r: float = 15.0, epsilon_rf: float = 0.0):
    """-> (f / eps_r, k_rf, c_rf)"""
    if epsilon_rf == 0.0:
        k_rf = 1.0 / (2.0 * r_cut**3)
    else:
        k_rf = (epsilon_rf - epsilon_r) / ((2.0 * epsilon_rf + epsilon_r) * r_cut**3)
    return F_ELEC / epsilon_r, k_rf, 1.0 / r_cut + k_rf * r_cut**2


def pair_v(r, qq, r_cut, epsilon_r=15.0, epsilon_rf=0.0, excluded=False):
    """V(r) and dV/dr of one pair with charge product ``qq`` (no cut-off test)."""
    pref, k_rf, c_rf = constants(r_cut, epsilon_r, epsilon_rf)
    r = np.asarray(r, dtype=np.float64)
    if excluded:
        return pref * qq * (k_rf * r * r - c_rf), pref * qq * 2.0 * k_rf * r
    return pref * qq * (1.0 / r + k_rf * r * r - c_rf), pref * qq * (2.0 * k_rf * r - 1.0 / (r * r))


def coulomb(pos, box, charges, bonds, r_cut, epsilon_r=15.0, epsilon_rf=0.0) -> dict:
    """One frame: pos (n, 3), box (3,), charges (n,), bonds (nb, 2) - the exclusions.

    -> dict: ``energy`` {pair, excluded, self}, ``forces`` {pair, excluded} (n, 3) = -dU/dx, ``virial`` {pair, excluded}
    (3,), and the totals ``e``, ``f``, ``w``."""
    x = np.asarray(pos, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(3)
    q = np.asarray(charges, dtype=np.float64)
    n = x.shape[0]
    pref, k_rf, c_rf = constants(r_cut, epsilon_r, epsilon_rf)
    idx = np.nonzero(q != 0.0)[0]  # (an uncharged bead contributes to no pair and to no sum)
    excl = np.zeros((n, n), dtype=bool)
    b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    excl[b[:, 0], b[:, 1]] = excl[b[:, 1], b[:, 0]] = True
    energy = {"pair": 0.0, "excluded": 0.0, "self": -0.5 * pref * c_rf * float((q * q).sum())}
    forces = {"pair": np.zeros((n, 3)), "excluded": np.zeros((n, 3))}
    virial = {"pair": np.zeros(3), "excluded": np.zeros(3)}
    if idx.size >= 2:
        a, c = np.triu_indices(idx.size, k=1)
        i, j = idx[a], idx[c]
        d = x[i] - x[j]
        d = d - box * np.round(d / box)
        r = np.sqrt((d * d).sum(1))
        inside = r < r_cut
        for part, sel in (("pair", inside & ~excl[i, j]), ("excluded", inside & excl[i, j])):
            ii, jj, dd, rr = i[sel], j[sel], d[sel], r[sel]
            qq = q[ii] * q[jj]
            if part == "pair":
                v = pref * qq * (1.0 / rr + k_rf * rr * rr - c_rf)
                dvdr = pref * qq * (2.0 * k_rf * rr - 1.0 / (rr * rr))
            else:
                v = pref * qq * (k_rf * rr * rr - c_rf)
                dvdr = pref * qq * 2.0 * k_rf * rr
            energy[part] = float(v.sum())
            g = (dvdr / rr)[:, None] * dd  # dV/dx_i
            np.add.at(forces[part], ii, -g)
            np.add.at(forces[part], jj, g)
            virial[part] = -((dvdr / rr)[:, None] * dd * dd).sum(0)
    return {"energy": energy, "forces": forces, "virial": virial, "e": sum(energy.values()),
            "f": forces["pair"] + forces["excluded"], "w": virial["pair"] + virial["excluded"]}
