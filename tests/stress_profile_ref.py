"""The lateral pressure profile of a MARTINI frame restated in fp64 NumPy, O(n^2): the pin of mythos_amd/csrc/stress_profile.hip
(tests/test_gpu_stress_profile.py), itself pinned by tests/test_stress_profile_cpu.py against the strain virial of
tests/martini_npt_ref.py.  Definitions: DESIGN section 3.5q.

``bead_shares``   w_i (n, 3) per term: an LJ pair, a bond, a reaction-field pair and an excluded reaction-field pair give
                  -1/2 g dx_d^2 to either bead (g = (dV/dr) / r), an angle -u_d dU/dx_id to its first and -v_d dU/dx_kd to its
                  last bead, nothing to its centre; minimum-image vectors.  Parameters as ``martini_npt_ref.strain_virial``
                  takes them; the Coulomb constants are ``martini_rf_ref.constants``.
``slab_index``    the slab of a stored z, fixed to the box or centred on a midpoint.
``raw_rows``      (n_bins, 4) count, W_x, W_y, W_z per slab, or (n_bins, 13) with the four terms apart.
``pressures`` / ``surface_tension``  the units of the Python layer.
``cases``         the systems of the GPU tests, with the assertion that no bead lies within 1e-6 slab thicknesses of a slab
                  edge - so that slab counts compare exactly.
"""

from __future__ import annotations

import functools

import numpy as np

from tests import martini_rf_ref as RF

BAR = 16.6053907  # kJ/mol/nm^3 -> bar
TERMS = ("lj", "bond", "angle", "coulomb")


def _image(d, box):
    return d - box * np.round(d / box)


def bead_shares(pos, box, types, sigma, eps, bonds, bond_k, bond_r0, angles, angle_k, angle_t0, use_g96, charges=None, r_cut=1.1,
                epsilon_r=15.0, epsilon_rf=0.0) -> dict:
    """-> {term: (n, 3) float64} in kJ/mol."""
    x = np.asarray(pos, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64).reshape(3)
    n = x.shape[0]
    types = np.asarray(types, dtype=np.int64)
    sigma, eps = np.asarray(sigma, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    angles = np.asarray(angles, dtype=np.int64).reshape(-1, 3)
    out = {t: np.zeros((n, 3)) for t in TERMS}

    excl = np.zeros((n, n), dtype=bool)
    excl[bonds[:, 0], bonds[:, 1]] = excl[bonds[:, 1], bonds[:, 0]] = True
    d = _image(x[:, None, :] - x[None, :, :], box)  # (n, n, 3): bead i minus bead j
    r2 = (d * d).sum(-1)
    np.fill_diagonal(r2, np.inf)
    inside = r2 < r_cut * r_cut
    r2s = np.where(inside, r2, 1.0)
    # Lennard-Jones: V = 4 eps (s12 - s6) + const, (dV/dr) / r = -24 eps (2 s12 - s6) / r^2
    s6 = (sigma[types[:, None], types[None, :]] ** 2 / r2s) ** 3
    g = -24.0 * eps[types[:, None], types[None, :]] * (2.0 * s6 * s6 - s6) / r2s
    g = np.where(inside & ~excl, g, 0.0)
    out["lj"] = (-0.5 * g[:, :, None] * d * d).sum(1)
    # reaction field: V = pref qq (1/r + k_rf r^2 - c_rf), an excluded pair without the 1/r
    if charges is not None and np.any(np.asarray(charges) != 0.0):
        q = np.asarray(charges, dtype=np.float64)
        pref, k_rf, _ = RF.constants(r_cut, epsilon_r, epsilon_rf)
        qq = pref * q[:, None] * q[None, :]
        gc = qq * np.where(excl, 2.0 * k_rf, 2.0 * k_rf - r2s ** -1.5)
        gc = np.where(inside, gc, 0.0)
        out["coulomb"] = (-0.5 * gc[:, :, None] * d * d).sum(1)
    # bonds: V = 1/2 k (r - r0)^2
    if bonds.shape[0]:
        db = _image(x[bonds[:, 0]] - x[bonds[:, 1]], box)
        r = np.sqrt((db * db).sum(1))
        gb = np.asarray(bond_k, dtype=np.float64) * (r - np.asarray(bond_r0, dtype=np.float64)) / r
        share = -0.5 * gb[:, None] * db * db
        np.add.at(out["bond"], bonds[:, 0], share)
        np.add.at(out["bond"], bonds[:, 1], share)
    # angles i - j - k: u = x_i - x_j, v = x_k - x_j, c = cos theta
    if angles.shape[0]:
        u = _image(x[angles[:, 0]] - x[angles[:, 1]], box)
        v = _image(x[angles[:, 2]] - x[angles[:, 1]], box)
        nu, nv = np.sqrt((u * u).sum(1)), np.sqrt((v * v).sum(1))
        c = (u * v).sum(1) / (nu * nv)
        k, t0 = np.asarray(angle_k, dtype=np.float64), np.asarray(angle_t0, dtype=np.float64)
        if use_g96:
            dudc = k * (c - np.cos(t0))  # U = 1/2 k (c - c0)^2
        else:
            cr = np.cross(u, v)
            sn = np.sqrt((cr * cr).sum(1)) / (nu * nv)
            dudc = -k * (np.arctan2(sn, c) - t0) / sn  # U = 1/2 k (theta - theta0)^2, dtheta/dc = -1 / sin
        dcdu = (v / nv[:, None] - c[:, None] * u / nu[:, None]) / nu[:, None]
        dcdv = (u / nu[:, None] - c[:, None] * v / nv[:, None]) / nv[:, None]
        np.add.at(out["angle"], angles[:, 0], -u * dudc[:, None] * dcdu)
        np.add.at(out["angle"], angles[:, 2], -v * dudc[:, None] * dcdv)
    return out


def midpoint(pos, index) -> float:
    """The mean stored z of the beads ``index``."""
    return float(np.asarray(pos, dtype=np.float64)[np.asarray(index, dtype=np.int64), 2].mean())


def slab_coordinate(z, lz, mid=None):
    """u n_bins is the slab before flooring: u in [0, 1), the fraction of the box (``mid`` None) or of the box centred on
    ``mid``, shifted by 1/2."""
    z = np.asarray(z, dtype=np.float64)
    if mid is None:
        t = z / lz
        return t - np.floor(t)
    t = (z - mid) / lz
    return (t - np.floor(t + 0.5)) + 0.5


def slab_index(z, lz, n_bins, mid=None):
    """bin = floor(u n_bins), clamped to [0, n_bins - 1] (u can round to 1, and u + 1/2 below 0)."""
    s = slab_coordinate(z, lz, mid) * float(n_bins)
    return np.clip(np.floor(s).astype(np.int64), 0, n_bins - 1)


def raw_rows(pos, box, n_bins, *ff, center_index=None, by_term=False, **coulomb) -> np.ndarray:
    """One frame -> (n_bins, 4) count, W_xyz or (n_bins, 13) count, W_xyz of lj, bond, angle, coulomb.  ``ff``: types ...
    use_g96 as ``bead_shares`` takes them."""
    w = bead_shares(pos, box, *ff, **coulomb)
    box = np.asarray(box, dtype=np.float64).reshape(3)
    mid = None if center_index is None or len(center_index) == 0 else midpoint(pos, center_index)
    b = slab_index(np.asarray(pos, dtype=np.float64)[:, 2], box[2], n_bins, mid)
    row = np.zeros((n_bins, 13))
    np.add.at(row[:, 0], b, 1.0)
    for t, term in enumerate(TERMS):
        np.add.at(row[:, 1 + 3 * t:4 + 3 * t], b, w[term])
    if by_term:
        return row
    return np.concatenate([row[:, :1], row[:, 1:].reshape(n_bins, 4, 3).sum(1)], axis=1)


def pressures(raw, box, kT) -> np.ndarray:
    """(n_bins, 4) raw row -> (n_bins, 3) P_xx, P_yy, P_zz in bar: (n_b kT + W_d(b)) / (Lx Ly dz) x BAR."""
    raw, box = np.asarray(raw, dtype=np.float64), np.asarray(box, dtype=np.float64).reshape(3)
    v_slab = box.prod() / raw.shape[0]
    return (raw[:, :1] * kT + raw[:, 1:4]) / v_slab * BAR


def surface_tension(raw, box, kT) -> float:
    """bar nm: sum_b dz [P_zz(b) - 1/2 (P_xx(b) + P_yy(b))]."""
    p = pressures(raw, box, kT)
    dz = float(np.asarray(box, dtype=np.float64).reshape(3)[2]) / p.shape[0]
    return float((dz * (p[:, 2] - 0.5 * (p[:, 0] + p[:, 1]))).sum())


# ---- the systems of tests/test_gpu_stress_profile.py ----------------------------------------------------------------------

N_BINS = (1, 7, 64, 65, 200)
# martini_synth systems of three frames with their own boxes; stored coordinates up to two boxes outside (images)
CASES = {
    "n131": dict(n=131, box=(3.0, 3.5, 3.7), seed=4131, frames=3, images=2, box_jitter=0.01),      # odd, under one tile; non-cubic
    "n259": dict(n=259, box=(3.2, 3.6, 4.1), seed=4259, frames=3, images=2, box_jitter=0.01),      # partial last tile and workgroup
    "slab259": dict(n=259, box=(6.0, 6.2, 2.6), seed=4260, frames=3, images=1, box_jitter=0.01),   # a slab box, harmonic angles
    "q259": dict(n=259, box=(3.2, 3.6, 4.1), seed=4261, frames=3, images=2, box_jitter=0.01),      # charges on
    "n61": dict(n=61, box=(2.6, 2.8, 3.0), seed=4061, frames=3, images=1, box_jitter=0.01),        # the chunk-boundary system
}
ANGLE_KIND = {"slab259": 1}
EDGE_CLEARANCE = 1e-6  # of a slab thickness


def clearance(z, lz, n_bins, mid=None) -> float:
    """The smallest distance of any bead to a slab edge, in slab thicknesses."""
    s = slab_coordinate(z, lz, mid) * float(n_bins)
    return float(np.abs(s - np.round(s)).min())


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """-> dict(n, ff (types ... angle_t0), angle_kind, pos (3, n, 3), box (3, 3), charges or None, center (bead indices))."""
    from tests import martini_synth as S

    s = S.make(**CASES[name])
    S.check(s)
    n = s["n"]
    ff = tuple(s[k] for k in ("types", "sigma", "eps", "bonds", "bond_k", "bond_r0", "angles", "angle_k", "angle_t0"))
    charges = None
    if name.startswith("q"):
        rng = np.random.default_rng(CASES[name]["seed"])
        charges = rng.choice([-1.0, 0.0, 0.0, 0.5, 1.0], size=n)
        b = s["bonds"][:8]
        charges[b[:, 0]], charges[b[:, 1]] = 1.0, -1.0  # (bonded charged pairs: the excluded-pair term)
    center = np.arange(0, n, 3, dtype=np.int32)
    out = dict(n=n, ff=ff, angle_kind=ANGLE_KIND.get(name, 0), pos=s["pos"], box=s["box"], charges=charges, center=center)
    assert_clear_of_edges(out)
    return out


def assert_clear_of_edges(c, n_bins=N_BINS) -> None:
    """No bead within EDGE_CLEARANCE slab thicknesses of a slab edge, box-fixed and centred, in fp64 and as fp32 values."""
    for cast in (np.float64, np.float32):
        pos, box = c["pos"].astype(cast).astype(np.float64), c["box"].astype(cast).astype(np.float64)
        for f in range(pos.shape[0]):
            for mid in (None, midpoint(pos[f], c["center"])):
                for nb in n_bins:
                    if nb > 1:
                        assert clearance(pos[f, :, 2], box[f, 2], nb, mid) > EDGE_CLEARANCE, (f, nb, mid)


def promoted(c, fp32: bool) -> dict:
    """The case with every real rounded to fp32 and widened back (``fp32``), or as it is: what the kernels are given."""
    r = (lambda a: np.asarray(a).astype(np.float32).astype(np.float64)) if fp32 else (lambda a: np.asarray(a, dtype=np.float64))
    t, sg, ep, b, bk, br, an, ak, at = c["ff"]
    q = None if c["charges"] is None else r(c["charges"])
    return dict(c, ff=(t, r(sg), r(ep), b, r(bk), r(br), an, r(ak), r(at)), pos=r(c["pos"]), box=r(c["box"]), charges=q)


def reference_rows(c, n_bins, *, centered=False, by_term=True, frames=None) -> np.ndarray:
    """(F, n_bins, 13 or 4) of the case's frames."""
    fr = range(c["pos"].shape[0]) if frames is None else frames
    return np.stack([raw_rows(c["pos"][f], c["box"][f], n_bins, *c["ff"], c["angle_kind"] == 0,
                              center_index=c["center"] if centered else None, by_term=by_term, charges=c["charges"]) for f in fr])
