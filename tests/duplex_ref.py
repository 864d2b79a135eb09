"""numpy fp64 restatement of the reference's duplex-mechanics observables for this package's site conventions - TEST
INFRASTRUCTURE ONLY, the checker of mythos_amd/csrc/duplex_obs.hip:

    diameter.py:23-46          single_diameter          -> backbone_distance / diameter
    stretch_torsion.py:16-35   single_angle_xy          -> twist_xy
    stretch_torsion.py:77-95   single_extension_z       -> extension_z
    rmse.py:19-67              svd_align / single_rmse  -> rmsd (oxDNA length units: the Angstrom factor is the caller's)

Frames are (S, n, 3) centres and (S, n, 4) quaternions [w, x, y, z]; ``g3`` = (com_to_hb, backbone offset on a1, backbone
offset on a2 - for model 3 on a3), ``box`` a periodic box or None.
"""

from __future__ import annotations

import numpy as np

ANGSTROMS_PER_OXDNA_LENGTH = 8.518


def axes(q):
    q0, q1, q2, q3 = (q[..., k] for k in range(4))
    a1 = np.stack([q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 + q0 * q3), 2 * (q1 * q3 - q0 * q2)], axis=-1)
    a2 = np.stack([2 * (q1 * q2 - q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 + q0 * q1)], axis=-1)
    a3 = np.stack([2 * (q1 * q3 + q0 * q2), 2 * (q2 * q3 - q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3], axis=-1)
    return a1, a2, a3


def disp(a, b, box):
    """jax_md's displacement(a, b) = a - b, wrapped into the box if there is one."""
    d = a - b
    if box is None:
        return d
    side = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,))
    return np.mod(d + 0.5 * side, side) - 0.5 * side


def sites(center, quat, g3, model):
    """(backbone sites, base sites), each (S, n, 3)."""
    a1, a2, a3 = axes(np.asarray(quat, dtype=np.float64))
    c = np.asarray(center, dtype=np.float64)
    second = a3 if model == 3 else a2
    k2 = g3[2] if model >= 2 else 0.0
    return c + g3[1] * a1 + k2 * second, c + g3[0] * a1


def backbone_distance(center, quat, pairs, g3, model, box=None):
    """(S,) mean over the pairs of |disp(back_i, back_j)| - the diameter without sigma_backbone and units."""
    back, _ = sites(center, quat, g3, model)
    pairs = np.asarray(pairs).reshape(-1, 2)
    d = disp(back[:, pairs[:, 0]], back[:, pairs[:, 1]], box)
    return np.linalg.norm(d, axis=-1).mean(axis=1)


def diameter(center, quat, pairs, g3, model, sigma_backbone, box=None):
    return (backbone_distance(center, quat, pairs, g3, model, box) + sigma_backbone) * ANGSTROMS_PER_OXDNA_LENGTH


def extension_z(center, bp1, bp2, box=None):
    c = np.asarray(center, dtype=np.float64)
    (a1, b1), (a2, b2) = bp1, bp2
    m1 = c[:, a1] + disp(c[:, b1], c[:, a1], box) / 2
    m2 = c[:, a2] + disp(c[:, b2], c[:, a2], box) / 2
    return np.abs(disp(m2, m1, box)[:, 2])


def twist_xy(center, quat, quartets, g3, model, box=None):
    _, base = sites(center, quat, g3, model)
    qs = np.asarray(quartets).reshape(-1, 2, 2)
    bb1 = disp(base[:, qs[:, 0, 1]], base[:, qs[:, 0, 0]], box)[..., :2]
    bb2 = disp(base[:, qs[:, 1, 1]], base[:, qs[:, 1, 0]], box)[..., :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        bb1 = bb1 / np.linalg.norm(bb1, axis=-1, keepdims=True)
        bb2 = bb2 / np.linalg.norm(bb2, axis=-1, keepdims=True)
    return np.arccos(np.clip((bb1 * bb2).sum(-1), -1.0, 1.0)).sum(axis=1)


def rmsd(target, center):
    """(S,) after svd_align (rmse.py:19-53): the target is centred here as RMSE.__call__ does (rmse.py:110-113)."""
    t = np.asarray(target, dtype=np.float64)
    t = t - t.mean(axis=0)
    out = []
    for x in np.asarray(center, dtype=np.float64):
        x = x - x.mean(axis=0)
        u, _, vt = np.linalg.svd(x.T @ t)
        rot = (vt.T @ u.T).T
        if np.linalg.det(rot) < 0:
            vt = vt.copy()
            vt[2] = -vt[2]
            rot = (vt.T @ u.T).T
        out.append(np.sqrt((np.linalg.norm(x @ rot - t, axis=1) ** 2).mean()))
    return np.array(out)
