"""NumPy restatement of the membrane definitions: what LiPyphilic's AssignLeaflets,
MembThickness and AreaPerLipid do at their defaults (n_bins = 1), as the reference calls them in
mythos/observables/membrane_thickness.py:33-43 and area_per_lipid.py:31-41.  The checker of the membrane tests; it is
itself held to the ten known answers of the reference's tests (tests/test_membrane_cpu.py).

Selections are plain: a tuple of bead names, optionally restricted to one residue name - written here from the names,
not through the package's parser.
"""

from __future__ import annotations

import numpy as np


def mask(top, names, resname=None) -> np.ndarray:
    m = np.isin(np.asarray(top.atom_names), list(names))
    if resname is not None:
        m &= np.asarray(top.residue_names) == resname
    return m


def membrane(x, box, residue_index, lipid_mask, thick_mask=None) -> dict:
    """Per frame, in nm: thickness, apl, mid, n_up, n_lo, z_up, z_lo (S,), leaflets (S, n_lipids) int8, lipid_z
    (S, n_lipids) and the lipids' residue numbers."""
    x, box, resid = np.asarray(x, dtype=np.float64), np.asarray(box, dtype=np.float64).reshape(-1, 3), np.asarray(residue_index)
    s = x.shape[0]
    if box.shape[0] == 1:
        box = np.repeat(box, s, axis=0)
    sel = np.flatnonzero(lipid_mask)
    residues = np.unique(resid[sel])
    members = [sel[resid[sel] == r] for r in residues]
    thick = np.flatnonzero(thick_mask) if thick_mask is not None else np.zeros(0, dtype=np.int64)
    lipid_of = {int(r): k for k, r in enumerate(residues)}
    thick_lipid = np.array([lipid_of[int(resid[b])] for b in thick], dtype=np.int64)
    out = {k: np.full(s, np.nan) for k in ("thickness", "apl", "mid", "n_up", "n_lo", "z_up", "z_lo")}
    out["leaflets"] = np.zeros((s, len(residues)), dtype=np.int8)
    out["lipid_z"] = np.zeros((s, len(residues)))
    out["residues"] = residues
    for f in range(s):
        z = x[f, :, 2]
        mid = z[sel].mean()  # over beads, not over lipids
        lz = np.array([z[m].mean() for m in members])  # unweighted
        leaf = np.where(lz > mid, 1, -1)  # a tie goes to -1
        n_up, n_lo = int((leaf == 1).sum()), int((leaf == -1).sum())
        tl = leaf[thick_lipid] if thick.size else np.zeros(0, dtype=np.int64)
        up, lo = thick[tl == 1], thick[tl == -1]
        z_up = z[up].mean() if up.size else np.nan
        z_lo = z[lo].mean() if lo.size else np.nan
        out["thickness"][f] = z_up - z_lo
        out["apl"][f] = box[f, 0] * box[f, 1] * ((n_up > 0) + (n_lo > 0)) / len(residues)
        out["mid"][f], out["n_up"][f], out["n_lo"][f], out["z_up"][f], out["z_lo"][f] = mid, n_up, n_lo, z_up, z_lo
        out["leaflets"][f], out["lipid_z"][f] = leaf, lz
    return out
