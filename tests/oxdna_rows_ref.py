"""The oxDNA neighbour-row contract in NumPy, fp64 (no GPU): which unbonded pairs a row must hold, which it may hold,
and in which segment - the brute-force reference of tests/test_gpu_oxdna_rows.py, held to what is relied on by
tests/test_oxdna_rows_ref_cpu.py.  DESIGN.md, "The neighbour-row contract", states the contract in words.

Two classifications of every unordered pair (i, j) that is not bonded:

``must``  what the physics needs, by the parameter vector of the pair's OWN type (oxNA: DNA-DNA, RNA-RNA, hybrid) and the
          nucleotides' real sites (backbone c + GEO_BACK_A1 a1 + GEO_BACK_A2 a2 - a3 for oxRNA2 and the RNA nucleotides
          of oxNA -, base c + GEO_BASE a1, stack c + GEO_STACK a1):
          close  centre distance < r_cut + skin and one of: base-base < max(HYDR_RCHIGH, CRST_RCHIGH, NEXC_BASE_RC) +
                 skin, stack-stack < CXST_RCHIGH + skin, backbone-base (either way) < max(NEXC_BACK_BASE_RC,
                 NEXC_BASE_BACK_RC) + skin;
          far    not close and backbone-backbone < max(NEXC_BACKBONE_RC, DH_RCUT from oxDNA2 on) + skin.
``may``   the builder's documented criterion (mythos_amd/csrc/neighbors.hip, SiteCrit and build_cells_typed): the largest
          range over the system's vectors, base and stack sites at the MEAN offset of the two geometries along a1 with
          the ranges widened by the distance a real site can be from there, the real backbone offsets, the centre range
          of the close segment (oxdna_close_range + skin) and of the list (r_cut + skin).

For models 1-3 the two are the same sets (up to the centre ranges, which hold whenever a site range does); for oxNA
must is a subset of may: must-close of may-close, must-listed of may-listed (a must-far pair can be may-close, where
the wider ranges of another vector reach it; the close segment evaluates the backbone-backbone terms as well, so nothing
is lost there).  A row is right when its close segment holds every must-close pair and nothing outside may-close, its
far segment nothing outside may-far, and every must-far pair is in one of the two.

Margin band: a pair whose class would change if one of its deciding distances moved by ``band`` is reported in
``band`` and left out of every comparison (1e-9 for fp64 inputs, 1e-4 for fp32 ones - coordinates below 64 round to
3.8e-6, a site distance carries about six such roundings and an axis derived from an fp32 quaternion; 1e-4 is four times
that sum).  For fp32 the reference runs on the inputs rounded to fp32 and cast back up (``as_seen_by``).  At most
``BAND_CAP`` of a case's listed pairs may lie in a band: a condition on the inputs, checked with the reference alone.

``centre_rows`` is the energy-path builder (OxdnaSystem.build_neighbors), which knows no sites: listed iff the centre
distance is under r_list, close iff under min(r_list, close range + skin).

The second half of the file holds the systems of the GPU tests (``case``), so that the CPU test can check their coverage
conditions - which builder a case takes, row lengths, non-empty classes, band cap - without a GPU.
"""

from __future__ import annotations

import dataclasses as dc
import functools

import numpy as np

BAND = {"f64": 1e-9, "f32": 1e-4}
BAND_CAP = 0.005
R_CUT = 3.3
BONDED = 4            # slots at the head of every row
ROLE_Q = 1 << 30
INDEX_MASK = ROLE_Q - 1
CELLS_FROM = 512      # cell_grid (mythos_amd/csrc/cell_list.h): all pairs under 512 particles ...
CELLS_PER_EDGE = 3    # ... or under three cells of the list range on a periodic edge


# ---- geometry -----------------------------------------------------------------------------------------------------

def quat_axes(q):
    """(a1, a2, a3), each (N, 3), of unit quaternions (the convention of oracle/oxdna_oracle.py:quat_to_axes)."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    q0, q1, q2, q3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    a1 = np.stack([q0**2 + q1**2 - q2**2 - q3**2, 2 * (q1 * q2 + q0 * q3), 2 * (q1 * q3 - q0 * q2)], axis=1)
    a2 = np.stack([2 * (q1 * q2 - q0 * q3), q0**2 - q1**2 + q2**2 - q3**2, 2 * (q2 * q3 + q0 * q1)], axis=1)
    a3 = np.stack([2 * (q1 * q3 + q0 * q2), 2 * (q2 * q3 - q0 * q1), q0**2 - q1**2 - q2**2 + q3**2], axis=1)
    return a1, a2, a3


def as_seen_by(x, dtype: str):
    """The array as a kernel of that precision receives it, in float64."""
    x = np.asarray(x, dtype=np.float64)
    return x.astype(np.float32).astype(np.float64) if dtype == "f32" else x


def _pair_dist(a, b, box):
    """(N, N): |b_j - a_i|, minimum image in a box."""
    d = b[None, :, :] - a[:, None, :]
    if box is not None:
        L = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,))
        d = d - L * np.rint(d / L)
    return np.sqrt((d * d).sum(-1))


def param_sets(flat, names, model: int):
    """The flat vector(s) by name: one dict, or (oxNA) three - oxDNA2, oxRNA2, hybrid."""
    flat = np.asarray(flat, dtype=np.float64).reshape(-1)
    k = 3 if model == 4 else 1
    assert flat.shape[0] == k * len(names), (flat.shape, len(names))
    return [dict(zip(names, flat[s * len(names):(s + 1) * len(names)])) for s in range(k)]


def _excluded(n, bonded):
    ex = np.eye(n, dtype=bool)
    b = np.asarray(bonded, dtype=np.int64).reshape(-1, 2)
    ex[b[:, 0], b[:, 1]] = True
    ex[b[:, 1], b[:, 0]] = True
    return ex


@dc.dataclass
class Rows:
    """One classification: symmetric (N, N) bool matrices, False on the diagonal and on bonded pairs.  ``band``: the
    class is not decided within the margin; ``dist`` / ``thr``: the deciding distances and their thresholds by name
    (thresholds are scalars or (N, N)), for the failure messages."""

    close: np.ndarray
    far: np.ndarray
    band: np.ndarray
    dist: dict
    thr: dict

    @property
    def listed(self):
        return self.close | self.far

    def describe(self, i, j):
        out = []
        for k, d in self.dist.items():
            t = self.thr[k]
            out.append(f"{k} {d[i, j]:.7f} (< {float(t[i, j] if np.ndim(t) else t):.7f})")
        return ", ".join(out)


def _classify(dist, thr, band, excluded, centre_close, centre_far):
    """close = centre_close test and any site test; far = (centre_far test and) not close and the bb test.  Every test
    is taken at its threshold, band below it (certainly inside) and band above it (possibly inside); a pair whose class
    differs between the two extremes is in the band."""
    def test(key, shift):
        return dist[key] < thr[key] + shift

    def close_of(shift):  # every test of the close class lets a pair IN: one shift moves them all the same way
        site = test("base-base", shift) | test("stack-stack", shift) | test("back_i-base_j", shift) | test("base_i-back_j", shift)
        return site & test(centre_close, shift)

    close = close_of(0.0)
    close_min, close_max = close_of(-band), close_of(band)

    def far_of(cl, shift):
        f = ~cl & test("back-back", shift)
        return f & test(centre_far, shift) if centre_far else f

    far = far_of(close, 0.0)
    far_min, far_max = far_of(close_max, -band), far_of(close_min, band)
    unsure = (close_min != close_max) | (far_min != far_max)
    keep = ~excluded
    return Rows(close & keep, far & keep, unsure & keep, dist, thr)


def site_rows(center, quat, model: int, flat, names, *, is_rna=None, box=None, bonded=(), r_cut=R_CUT, skin, band):
    """(must, may) of one frame: two ``Rows``."""
    c = np.asarray(center, dtype=np.float64)
    n = c.shape[0]
    P = param_sets(flat, names, model)
    rna = np.zeros(n, dtype=bool) if (model != 4 or is_rna is None) else np.asarray(is_rna, dtype=bool)
    a1, a2, a3 = quat_axes(quat)
    own = rna.astype(np.int64) if model == 4 else np.zeros(n, dtype=np.int64)  # the vector that holds a nucleotide's geometry

    def geo(key):
        return np.array([P[s][key] for s in range(min(len(P), 2))])[own]

    on_a3 = rna | (model == 3)
    k2 = geo("GEO_BACK_A2") if model >= 2 else np.zeros(n)
    back_off = geo("GEO_BACK_A1")[:, None] * a1 + k2[:, None] * np.where(on_a3[:, None], a3, a2)
    back = c + back_off
    base = c + geo("GEO_BASE")[:, None] * a1
    stack = c + geo("GEO_STACK")[:, None] * a1
    excluded = _excluded(n, bonded)
    r_list = r_cut + skin
    centre = _pair_dist(c, c, box)

    # ---- must: the pair's own vector, the real sites
    if model == 4:
        vec = np.where(rna[:, None] & rna[None, :], 1, np.where(~rna[:, None] & ~rna[None, :], 0, 2))
    else:
        vec = np.zeros((n, n), dtype=np.int64)

    def own_range(fn):
        return np.array([fn(p) for p in P])[vec]

    dist = {"centre": centre, "base-base": _pair_dist(base, base, box), "stack-stack": _pair_dist(stack, stack, box),
            "back_i-base_j": _pair_dist(back, base, box), "base_i-back_j": _pair_dist(base, back, box),
            "back-back": _pair_dist(back, back, box)}
    thr = {"centre": r_list,
           "base-base": own_range(lambda p: max(p["HYDR_RCHIGH"], p["CRST_RCHIGH"], p["NEXC_BASE_RC"])) + skin,
           "stack-stack": own_range(lambda p: p["CXST_RCHIGH"]) + skin,
           "back_i-base_j": own_range(lambda p: max(p["NEXC_BACK_BASE_RC"], p["NEXC_BASE_BACK_RC"])) + skin,
           "back-back": own_range(lambda p: max(p["NEXC_BACKBONE_RC"], p["DH_RCUT"] if model >= 2 else 0.0)) + skin}
    thr["base_i-back_j"] = thr["back_i-base_j"]
    must = _classify(dist, thr, band, excluded, "centre", None)

    # ---- may: the builder's criterion
    def mx(key):
        return max(p[key] for p in P)

    Pd, Pr = P[0], P[1 if len(P) > 1 else 0]
    slack_ba, slack_st = abs(Pd["GEO_BASE"] - Pr["GEO_BASE"]), abs(Pd["GEO_STACK"] - Pr["GEO_STACK"])
    mbase = c + 0.5 * (Pd["GEO_BASE"] + Pr["GEO_BASE"]) * a1
    mstack = c + 0.5 * (Pd["GEO_STACK"] + Pr["GEO_STACK"]) * a1
    mdist = {"centre-close": centre, "centre": centre, "base-base": _pair_dist(mbase, mbase, box),
             "stack-stack": _pair_dist(mstack, mstack, box), "back_i-base_j": _pair_dist(back, mbase, box),
             "base_i-back_j": _pair_dist(mbase, back, box), "back-back": dist["back-back"]}
    rbb = mx("NEXC_BACKBONE_RC")
    if model >= 2:
        rbb = max(rbb, mx("DH_RCUT"))
    mthr = {"centre-close": min(r_list, close_range(P, model) + skin), "centre": r_list,
            "base-base": max(mx("HYDR_RCHIGH"), mx("CRST_RCHIGH"), mx("NEXC_BASE_RC")) + slack_ba + skin,
            "stack-stack": mx("CXST_RCHIGH") + slack_st + skin,
            "back_i-base_j": max(mx("NEXC_BACK_BASE_RC"), mx("NEXC_BASE_BACK_RC")) + 0.5 * slack_ba + skin,
            "back-back": min(r_list, rbb + skin)}
    mthr["base_i-back_j"] = mthr["back_i-base_j"]
    may = _classify(mdist, mthr, band, excluded, "centre-close", "centre")
    return must, may


def close_range(P, model: int) -> float:
    """oxdna_close_range (mythos_amd/csrc/mythos_internal.h): the largest centre distance at which anything but the
    backbone-backbone terms can act."""
    geo = P[:2]
    off_back = max(np.sqrt(p["GEO_BACK_A1"] ** 2 + (p["GEO_BACK_A2"] ** 2 if model >= 2 else 0.0)) for p in geo)
    off_base = max(abs(p["GEO_BASE"]) for p in geo)
    off_stack = max(abs(p["GEO_STACK"]) for p in geo)

    def mx(key):
        return max(p[key] for p in P)

    r = max(mx("NEXC_BACK_BASE_RC"), mx("NEXC_BASE_BACK_RC")) + off_back + off_base
    r = max(r, mx("NEXC_BASE_RC") + 2 * off_base, max(mx("HYDR_RCHIGH"), mx("CRST_RCHIGH")) + 2 * off_base, mx("CXST_RCHIGH") + 2 * off_stack)
    return r * (1.0 + 1e-6)


def centre_rows(center, *, box=None, bonded=(), r_list, r_close, band) -> Rows:
    """The energy-path builder: listed iff centre distance < r_list, close iff < min(r_list, r_close)."""
    c = np.asarray(center, dtype=np.float64)
    d = _pair_dist(c, c, box)
    rc = min(r_list, r_close)
    keep = ~_excluded(c.shape[0], bonded)
    close, listed = d < rc, d < r_list
    unsure = (np.abs(d - rc) < band) | (np.abs(d - r_list) < band)
    return Rows(close & keep, listed & ~close & keep, unsure & keep, {"centre-close": d, "centre": d}, {"centre-close": rc, "centre": r_list})


# ---- rows read back from the device --------------------------------------------------------------------------------

def decode(rows, ln, close):
    """(close (N, N) bool, far (N, N) bool, problems) of OxdnaSystem.rows(): entry = index | role bit, the role bit set
    iff index < i; ``problems`` lists entries that break that, repeat or leave the range."""
    n = rows.shape[0]
    gc, gf, bad = np.zeros((n, n), dtype=bool), np.zeros((n, n), dtype=bool), []
    for i in range(n):
        ent = rows[i, BONDED:ln[i]]
        idx = ent & INDEX_MASK
        if (ent < 0).any() or (idx >= n).any() or (idx == i).any() or len(set(idx.tolist())) != len(idx):
            bad.append((i, "range / repeat", ent.tolist()))
            continue
        if (((ent & ROLE_Q) != 0) != (idx < i)).any():
            bad.append((i, "role bit", ent.tolist()))
        k = close[i] - BONDED
        gc[i, idx[:k]] = True
        gf[i, idx[k:]] = True
    return gc, gf, bad


def contract_failures(got_close, got_far, must: Rows, may: Rows, limit=8):
    """Messages for every way the decoded rows break  must <= rows <= may  (band pairs excepted), pair by pair with the
    deciding distances and thresholds; empty when the rows are right."""
    sure_must, sure_may = ~must.band, ~may.band
    checks = (
        ("must-close pair in the FAR segment", must.close & sure_must & got_far, must),
        ("must-close pair missing", must.close & sure_must & ~got_close & ~got_far, must),
        # (in the close segment a pair gets every term, the backbone-backbone ones too: where may-close is wider than
        # must-close - oxNA - a must-far pair may sit there; for models 1-3 the next line but one catches it)
        ("must-far pair missing", must.far & sure_must & ~got_far & ~got_close, must),
        ("close entry outside may-close", got_close & ~may.close & sure_may, may),
        ("far entry outside may-far", got_far & ~may.far & sure_may, may),
        ("row i holds j in its close segment, row j does not hold i there", got_close & ~got_close.T, may),
        ("row i holds j in its far segment, row j does not hold i there", got_far & ~got_far.T, may),
    )
    out = []
    for what, wrong, ref in checks:
        ii, jj = np.nonzero(wrong)
        for i, j in list(zip(ii.tolist(), jj.tolist()))[:limit]:
            out.append(f"{what}: ({i}, {j}): {ref.describe(i, j)}")
        if len(ii) > limit:
            out.append(f"{what}: {len(ii) - limit} more")
    return out


def uses_cells(n: int, box, r_list: float) -> bool:
    """cell_grid's rule: the cell kernel from 512 particles and three cells of the list range per periodic edge on."""
    if n < CELLS_FROM:
        return False
    return box is None or all(int(np.floor(e / r_list)) >= CELLS_PER_EDGE for e in np.broadcast_to(np.asarray(box, dtype=np.float64), (3,)))


def cell_occupancy(center, box, r_list: float):
    """Nucleotides per cell of the builder's grid (cell_of in cell_list.h): counts of the occupied cells."""
    c = np.asarray(center, dtype=np.float64)
    if box is None:
        cell = np.floor(c / r_list).astype(np.int64)
    else:
        L = np.broadcast_to(np.asarray(box, dtype=np.float64), (3,))
        nc = np.maximum(np.floor(L / r_list).astype(np.int64), 1)
        f = c / L
        cell = np.minimum(((f - np.floor(f)) * nc).astype(np.int64), nc - 1)
    _, counts = np.unique(cell, axis=0, return_counts=True)
    return counts


# ---- the systems of tests/test_gpu_oxdna_rows.py -----------------------------------------------------------------------

SALT = {1: 0.5, 2: 0.5, 3: 1.0, 4: 0.5}


HYBRID_GEOMETRY = {"GEO_BASE": 0.46, "GEO_STACK": 0.29}  # of the oxRNA2 (and hybrid) vector of the oxNA cases


@functools.lru_cache(maxsize=None)
def flat_for(model: int):
    """Default parameters of a model as the flat vector(s) of the C ABI (float64 numpy) and the entry names.  oxNA: the
    defaults put the base and stack sites of DNA and RNA at the same place along a1 (0.4, 0.34), which leaves the
    builder's slack terms at zero; the cases move the RNA sites (HYBRID_GEOMETRY) so that they are not."""
    from mythos_amd import _lib
    from mythos_amd.energy import flat_params as fp
    from mythos_amd.input import defaults
    from tests import helpers as H

    names = _lib.param_names()
    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    kw = dict(kt=sim["kT"], salt_conc=SALT[model], half_charged_ends=False)
    if model == 4:
        flat = fp.pack_flat_na1(fp.derive_flat_na1(cfg["dna"], cfg["rna"], cfg["drh"], **kw), names).detach().clone()
        for key, v in HYBRID_GEOMETRY.items():
            for s in (1, 2):
                flat[s * len(names) + names.index(key)] = v
    else:
        flat = fp.pack_flat(fp.derive_flat(model, cfg, **kw), names)
    return flat.detach().numpy().astype(np.float64), tuple(names)


def perturbed(c, q, seed: int, sigma: float = 0.05):
    """N(0, sigma) on the centres and a like tilt of a1, re-orthonormalised (the generators are regular lattices with
    degenerate distances: pairs would sit ON thresholds)."""
    from mythos_amd.input.trajectory import axes_to_quaternion

    rng = np.random.default_rng(seed)
    a1, _, a3 = quat_axes(q)
    c = np.asarray(c, dtype=np.float64) + sigma * rng.standard_normal(np.shape(c))
    a1 = a1 + sigma * rng.standard_normal(a1.shape)
    a1 /= np.linalg.norm(a1, axis=1, keepdims=True)
    a3 = a3 - (a3 * a1).sum(1, keepdims=True) * a1
    a3 /= np.linalg.norm(a3, axis=1, keepdims=True)
    return np.ascontiguousarray(c), np.ascontiguousarray(axes_to_quaternion(a1, a3))


@dc.dataclass(frozen=True)
class Case:
    name: str
    model: int
    top: object
    c: np.ndarray
    q: np.ndarray
    box: object          # (3,) array or None
    is_rna: object       # (N,) bool or None
    skin: float
    cells: bool          # the builder the case is meant to take
    r_cut: float = R_CUT

    @property
    def n(self):
        return self.c.shape[0]

    @property
    def r_list(self):
        return self.r_cut + self.skin

    def reference(self, dtype: str, c=None, q=None):
        """(must, may) at the case's frame, or at another one of the same system."""
        flat, names = flat_for(self.model)
        return site_rows(as_seen_by(self.c if c is None else c, dtype), as_seen_by(self.q if q is None else q, dtype), self.model,
                         flat, names, is_rna=self.is_rna, box=self.box, bonded=self.top.bonded_neighbors, r_cut=self.r_cut,
                         skin=self.skin, band=BAND[dtype])

    def centre_reference(self, dtype: str):
        flat, names = flat_for(self.model)
        return centre_rows(as_seen_by(self.c, dtype), box=self.box, bonded=self.top.bonded_neighbors, r_list=self.r_list,
                           r_close=close_range(param_sets(flat, names, self.model), self.model) + self.skin, band=BAND[dtype])


def _two_duplexes(model: int, apart: float):
    """Two 12 bp duplexes along z, their axes ``apart`` apart along x; the axis of the first lies in the plane x = 0."""
    from mythos_amd.input import topology
    from mythos_amd.utils import generators

    parts = [generators.ideal_duplex(12, model=model, seed=21 + k, origin=(apart * k, 4.0, 2.5)) for k in range(2)]
    top = topology.from_arrays(np.concatenate([p[0].seq for p in parts]).astype(np.int32), [12] * 4)
    return top, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def _tiled_hybrid(reps=(4, 4, 2), pitch=(3.4, 3.4, 7.0)):
    """The golden DNA-RNA helix on a lattice in free space: reps copies, the types tiled alongside."""
    from mythos_amd.input import topology
    from tests import helpers as H

    top, traj, _, is_rna = H.load_golden_na1("simple-helix-dna-rna")
    c0, q0 = np.array(traj.center[0], dtype=np.float64), np.array(traj.quaternions[0], dtype=np.float64)
    c0 = c0 - c0.mean(0)
    shifts = [np.array([ix, iy, iz]) * np.array(pitch) for ix in range(reps[0]) for iy in range(reps[1]) for iz in range(reps[2])]
    k = len(shifts)
    t = topology.from_arrays(np.tile(np.asarray(top.seq, dtype=np.int32), k), list(np.asarray(top.strand_counts)) * k)
    return t, np.concatenate([c0 + s for s in shifts]), np.tile(q0, (k, 1)), np.tile(np.asarray(is_rna, dtype=bool), k)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    from mythos_amd.utils import generators
    from tests import helpers as H
    from tests import oxdna_periodic_synth as S

    if name in ("duplex40-skin0.3", "duplex40-skin1.5"):
        top, c, q = generators.ideal_duplex(40, model=2, seed=3)
        c, q = perturbed(c, q, 40)
        return Case(name, 2, top, c, q, None, None, float(name.split("skin")[1]), False)
    if name == "two-duplexes-periodic":  # a box of two cells of the list range per edge; the first duplex lies across the face x = 0
        top, c, q = _two_duplexes(2, 3.0)
        c, q = perturbed(c, q, 12)
        box = np.array([10.0, 10.0, 10.0])
        return Case(name, 2, top, np.mod(c, box), q, box, None, 0.6, False)  # folded in: its two halves sit at opposite faces
    if name == "dna1-two-duplexes":  # backbones of the two within reach of each other, bases not: a far segment without Debye-Hueckel
        top, c, q = _two_duplexes(1, 2.6)
        c, q = perturbed(c, q, 1)
        return Case(name, 1, top, c, q, None, None, 0.6, False)
    if name in ("bundle512", "bundle516", "bundle512-skin1.5"):
        n_bp, n_dup = (43, 6) if name == "bundle516" else (32, 8)
        top, c, q = generators.duplex_bundle(n_bp, n_dup, spacing=3.2)
        c, q = perturbed(c, q, 2 * n_bp * n_dup)
        return Case(name, 2, top, c, q, None, None, 1.5 if name.endswith("skin1.5") else 0.6, True)
    if name in ("lattice576", "lattice576-wrapped"):
        top, c, q, box = S.duplex_lattice(13.0)
        c, q = perturbed(c, q, 576)
        # one box edge back along y: still unwrapped and across every face, and every coordinate stays below 64 (the
        # premise of the fp32 band)
        c = S.wrapped(c, box) if name.endswith("wrapped") else c - np.array([0.0, box[1], 0.0])
        return Case(name, 2, top, np.ascontiguousarray(c), q, box, None, 0.6, True)
    if name == "hybrid-helix":
        top, traj, _, is_rna = H.load_golden_na1("simple-helix-dna-rna")
        box = np.broadcast_to(np.asarray(traj.box_size, dtype=np.float64), (3,)).copy()
        return Case(name, 4, top, np.array(traj.center[0], dtype=np.float64), np.array(traj.quaternions[0], dtype=np.float64), box,
                    np.asarray(is_rna, dtype=bool), 0.6, False)
    if name == "hybrid-tiled":
        top, c, q, is_rna = _tiled_hybrid()
        c, q = perturbed(c, q, 4)
        return Case(name, 4, top, c, q, None, is_rna, 0.6, True)
    if name in ("dna1-helix", "rna2-helix"):
        model, gold = (1, "simple-helix") if name == "dna1-helix" else (3, "simple-helix-12bp")
        top, traj, _, _ = H.load_golden(model, gold)
        box = np.broadcast_to(np.asarray(traj.box_size, dtype=np.float64), (3,)).copy()
        return Case(name, model, top, np.array(traj.center[0], dtype=np.float64), np.array(traj.quaternions[0], dtype=np.float64), box, None, 0.6, False)
    raise KeyError(name)


ALL_PAIRS_CASES = ("duplex40-skin0.3", "duplex40-skin1.5", "two-duplexes-periodic", "hybrid-helix", "dna1-helix", "dna1-two-duplexes", "rna2-helix")
FREE_CELL_CASES = ("bundle512", "bundle516")
PERIODIC_CELL_CASES = ("lattice576", "lattice576-wrapped")
CELL_CASES = FREE_CELL_CASES + PERIODIC_CELL_CASES   # again with buckets of three places, and on the energy path
LONG_ROW_CASE = "bundle512-skin1.5"
SITE_CASES = ALL_PAIRS_CASES + CELL_CASES + (LONG_ROW_CASE, "hybrid-tiled")
SPILL_BUCKET_CAP = 3
