"""Branch-complete dimer poses for the oxDNA pair terms: the instrument, the pose builder, the fixture and the comparisons.

The force field is a product of piecewise functions (f1 .. f6, the smoothed FENE, the Debye-Hueckel term), each with a core
branch and one or two smoothing tails.  A *cell* is (term, factor, branch): ``("hydrogen_bonding", "f4#3", "low_tail")`` is
the low tail of the fourth f4 the hydrogen-bonding term calls.  Factors are named by term and call order.

 * ``Recorder`` replaces the oracle's piecewise functions with wrappers that note, per cell, which pairs land there - and
   can scale ONE branch of ONE factor (the mutation the sensitivity test applies).
 * ``reachable_cells`` keeps the cells whose branch interval meets the range of the argument (theta in [0, pi], cosines in
   [-1, 1], r > 0), from the parameters alone.
 * ``build_poses`` draws seeded perturbations of the ideal geometry of every term and uniform poses, evaluates them with the
   oracle and keeps, per cell, well-conditioned poses where that cell's own branch carries most of the force and a 1 % error
   in it shows most.
 * ``fixture_text`` / ``load_fixture``: tests/golden/branch_poses/model{1,2,3}.dat (tests/golden/make_branch_poses.py
   regenerates them); nothing samples at test time.
 * ``compare_*``: the comparisons of tests/test_gpu_oxdna_branches.py, shared with the sensitivity test of
   tests/test_oxdna_branch_poses_cpu.py, which feeds them a mutated oracle in place of a kernel.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

from mythos_amd.utils import generators
from oracle import oxdna_oracle as orc
from oracle.langevin_oracle import drift
from tests import helpers as H

MODELS = (1, 2, 3)
SALT = {1: 0.5, 2: 0.5, 3: 1.0}
HCE = {1: False, 2: True, 3: True}  # half-charged ends: the end flags of the fixture matter to the Debye term
K_LIVE = 4        # live poses every reachable cell must hold
K_SELECT = 6      # poses the builder keeps per cell (a margin over K_LIVE)
LIVE = 1e-3       # a term is live in a pose when its magnitude is above this
EXC_MAX = 20.0    # poses with a larger excluded-volume energy are not kept
GRID = 8.0
FIXTURE_DIR = H.GOLDEN / "branch_poses"
BONDED_TERMS = ("fene", "bonded_excluded_volume", "stacking")
PI = math.pi

# cells no draw reached: (model, term, factor, branch) -> one-line geometric reason.  Capped at 5 % of the reachable cells of
# a model; core branches cannot be waived (tests/test_oxdna_branch_poses_cpu.py holds both conditions).
_COAX_CLASH = ("stacking sites closer than 0.22 with theta1 inside its window (a1 of the two within 1 rad of parallel) put the base "
               "sites within about 0.28: base-base excluded volume of 40 or more (sigma 0.33, eps 2), above the limit of 20 - no "
               "eligible pose among 5 500 live draws in the branch")
WAIVERS: dict[tuple, str] = {
    (1, "coaxial_stacking", "f2#0", "low_tail"): _COAX_CLASH,
    (2, "coaxial_stacking", "f2#0", "low_tail"): _COAX_CLASH,
}

_PAIR_FUNCS = {
    "pair_fene": "fene", "pair_exc_vol_bonded": "bonded_excluded_volume", "pair_stacking": "stacking",
    "pair_stacking_rna2": "stacking", "pair_exc_vol_unbonded": "unbonded_excluded_volume",
    "pair_hydrogen_bonding": "hydrogen_bonding", "pair_cross_stacking": "cross_stacking", "pair_coaxial": "coaxial_stacking",
    "pair_debye": "debye",
}
INF = float("inf")


def _fl(x):
    return float(x.detach()) if isinstance(x, torch.Tensor) else float(x)


# branch -> open interval of the first argument, from the remaining arguments of the oracle's function
def _iv_f12(r_low, r_high, r_c_low, r_c_high, *_):
    return {"core": (_fl(r_low), _fl(r_high)), "low_tail": (_fl(r_c_low), _fl(r_low)), "high_tail": (_fl(r_high), _fl(r_c_high))}


def _iv_f3(r_star, r_c, *_):
    return {"core": (-INF, _fl(r_star)), "tail": (_fl(r_star), _fl(r_c))}


def _iv_f4(theta0, d_star, d_c, *_):
    t0, ds, dc = _fl(theta0), _fl(d_star), _fl(d_c)
    return {"core": (t0 - ds, t0 + ds), "low_tail": (t0 - dc, t0 - ds), "high_tail": (t0 + ds, t0 + dc)}


def _iv_f5(x_star, x_c, *_):
    return {"plateau": (0.0, INF), "core": (_fl(x_star), 0.0), "tail": (_fl(x_c), _fl(x_star))}


def _iv_f6(a, b):
    return {"core": (_fl(b), INF)}


_INTERVALS = {"f1": _iv_f12, "f2": _iv_f12, "f3": _iv_f3, "f4": _iv_f4, "f5": _iv_f5, "f6": _iv_f6}
# the range of the first argument: radii are positive, angles come out of acos, f5 takes a cosine
_ARG_RANGE = {"f1": (0.0, INF), "f2": (0.0, INF), "f3": (0.0, INF), "f4": (0.0, PI), "f5": (-1.0, 1.0), "f6": (0.0, PI),
              "fene": (0.0, INF), "dh": (0.0, INF)}
# the oxDNA1 form of the coaxial term calls its seventh f4 with 2 pi - theta1 (dna1/coaxial_stacking.py)
_ARG_RANGE_AT = {("coaxial_stacking", "f4#6"): (PI, 2.0 * PI)}


class Recorder:
    """Context manager: while it is open, the oracle's f1 .. f6, FENE and Debye-Hueckel pieces record the branch every pair
    takes.  ``masks[cell]`` is a boolean tensor over the pairs of the call (bonded pairs for the bonded terms, unbonded
    pairs otherwise), ``intervals[cell]`` the branch interval.  ``mutate=cell`` scales that branch of that factor by
    ``scale`` (value and every derivative with it).  ``probe=True`` multiplies every branch by a tensor of ones that autograd
    can differentiate by (``probes[cell]``, one entry per pair): dU/d(probe) is what that branch of that factor contributes to
    the energy of the pair.  The originals are put back on exit."""

    def __init__(self, mutate=None, scale=1.01, probe=False):
        self.mutate, self.scale, self.probe = mutate, scale, probe
        self.masks, self.intervals, self.probes = {}, {}, {}
        self._term, self._count, self._saved = None, {}, {}

    def _note(self, factor, branch, x, lo, hi, out):
        cell = (self._term, factor, branch)
        xd = x.detach()
        mask = (xd > lo) & (xd < hi)
        self.masks[cell], self.intervals[cell] = mask, (lo, hi)
        if cell == self.mutate:
            out = out * torch.where(mask, torch.full_like(out, self.scale), torch.ones_like(out))
        if self.probe:
            self.probes[cell] = torch.ones_like(out).requires_grad_(True)
            out = out * torch.where(mask, self.probes[cell], torch.ones_like(out))
        return out

    def _wrap_f(self, name, orig):
        def wrapped(x, *args):
            out = orig(x, *args)
            k = self._count.get(name, 0)
            self._count[name] = k + 1
            for branch, (lo, hi) in _INTERVALS[name](*args).items():
                out = self._note(f"{name}#{k}", branch, x, lo, hi, out)
            return out

        return wrapped

    def _wrap_pair(self, name, orig):
        term = _PAIR_FUNCS[name]

        def wrapped(p, s, *args):
            self._term, self._count = term, {}
            out = orig(p, s, *args)
            if term == "fene":
                bonded, disp = args
                r = orc._norm(disp(s.back[bonded[:, 0]], s.back[bonded[:, 1]]))
                eps, r0, delt, fmax = (_fl(p[k]) for k in ("eps_backbone", "r0_backbone", "delta_backbone", "fmax"))
                xmax = (-eps + math.sqrt(eps**2 + 4 * fmax**2 * delt**2)) / (2 * fmax)
                diff = orc.smooth_abs(r.detach() - r0)
                out = self._note("fene#0", "core", diff, -INF, xmax + 1e-300, out)
                self.intervals[(term, "fene#0", "core")] = (r0 - xmax, r0 + xmax)
                out = self._note("fene#0", "outer", diff, xmax, INF, out)
                self.intervals[(term, "fene#0", "outer")] = (r0 + xmax, INF)
            elif term == "debye":
                _, pairs, disp = args
                r = orc._norm(disp(s.back[pairs[:, 1]], s.back[pairs[:, 0]]))
                out = self._note("dh#0", "core", r, -INF, _fl(p["r_high"]), out)
                out = self._note("dh#0", "tail", r, _fl(p["r_high"]) - 1e-300, _fl(p["r_cut"]), out)
            return out

        return wrapped

    def __enter__(self):
        for name in _INTERVALS:
            self._saved[name] = getattr(orc, name)
            setattr(orc, name, self._wrap_f(name, self._saved[name]))
        for name in _PAIR_FUNCS:
            self._saved[name] = getattr(orc, name)
            setattr(orc, name, self._wrap_pair(name, self._saved[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(orc, name, fn)
        return False


def reachable_cells(intervals: dict) -> list:
    """The cells whose branch interval meets the range of their argument, sorted."""
    out = []
    for cell, (lo, hi) in intervals.items():
        term, factor, _ = cell
        a, b = _ARG_RANGE_AT.get((term, factor), _ARG_RANGE[factor.split("#")[0]])
        if max(lo, a) < min(hi, b):
            out.append(cell)
    return sorted(out)


@functools.lru_cache(maxsize=None)
def params(model: int):
    return H.oracle_params(model, half_charged_ends=HCE[model], salt=SALT[model])


def _rna_stacking_f5_dead(vector: str, angle: int, branches):
    """oxRNA2 stacking: f5 takes x = a2 . d and the f4 of theta9 / theta10 takes acos(-p . d), with d the unit backbone
    separation and p = p3 / p5 a body-fixed unit vector mostly along -a2 (rna2/stacking.py).  Where x is far enough
    below 0, -p . d is below cos(delta_theta_c): that f4, a factor of the same product, is zero.  -> check(rng, m) ->
    (x in one of ``branches`` of f5, the f4 there), on m uniform directions d given in the body frame."""

    def check(rng, m):
        g, p = params(3)["geometry"], params(3)["stacking"]
        d = torch.as_tensor(_unit(rng, m))
        x = d[:, 1]
        theta = torch.acos(orc.clamp(-(g[f"{vector}_x"] * d[:, 0] + g[f"{vector}_y"] * d[:, 1] + g[f"{vector}_z"] * d[:, 2])))
        f4 = orc.f4(theta, p[f"theta0_stack_{angle}"], p[f"delta_theta_star_stack_{angle}"], p[f"delta_theta_stack_{angle}_c"],
                    p[f"a_stack_{angle}"], p[f"b_stack_{angle}"])
        k = angle - 9  # theta9 goes with cos(phi2), theta10 with cos(phi1)
        iv = _iv_f5(p[f"neg_cos_phi{2 - k}_star_stack"], p[f"neg_cos_phi{2 - k}_c_stack"])
        inside = np.zeros(m, bool)
        for b in branches:
            inside |= ((x > iv[b][0]) & (x < iv[b][1])).numpy()
        return inside, f4.numpy()

    return check


# cells that are zero by construction, with the check that shows it (tests/test_oxdna_branch_poses_cpu.py runs it): another
# factor of the same product vanishes throughout the branch.  They count against the same 5 % as the waivers.
PROVEN_DEAD = {
    (3, "stacking", "f5#0", "core"): _rna_stacking_f5_dead("p5", 10, ("core",)),
    (3, "stacking", "f5#0", "tail"): _rna_stacking_f5_dead("p5", 10, ("tail",)),
    (3, "stacking", "f5#1", "tail"): _rna_stacking_f5_dead("p3", 9, ("tail",)),
}
# cells whose 1 % error the fp32 comparison cannot show, whatever poses are selected; fp32_blind_evidence is the check that
# tests/test_oxdna_branch_poses_cpu.py runs for each.  Exempt from the fp32 legs of the sensitivity test only.
_OXDNA1_MIRROR = ("oxDNA1, the f4 of 2 pi - theta1: inside this branch a1 of the two nucleotides is within 0.17 rad of parallel, and "
                  "every site of oxDNA1 is on the a1 line, so while the stacking sites are inside the range of f2 the backbone sites "
                  "are inside their excluded volume.  In every eligible live draw aimed there the force on a nucleotide is above 100 "
                  "beside a coaxial term below 0.17, and a 1 % error in this factor moves forces and torques by less than 1e-5 of them")
FP32_BLIND: dict[tuple, str] = {
    (1, "coaxial_stacking", "f4#6", "core"): _OXDNA1_MIRROR,
    (1, "coaxial_stacking", "f4#6", "high_tail"): _OXDNA1_MIRROR,
}


def fp32_blind_evidence(model: int, cell):
    """A fresh seeded pool of the draws aimed at theta1 near pi (family (d) of _candidates, 40 000 poses), its eligible live
    poses in ``cell`` -> (mutation_ratio of each, largest force component on a nucleotide of each, |term| of each)."""
    cand = _candidates(model, 1, 10_000, 10, theta1_only=True)
    terms, masks, _ = evaluate(cand)
    hit = np.nonzero(masks[cell] & eligible(terms) & (np.abs(terms[cell[0]]) > LIVE))[0]
    sub = cand.subset(hit)
    _, gc, _ = oracle_energy(sub)
    return mutation_ratio(sub, cell), np.abs(gc).max(1).reshape(-1, 2).min(1), np.abs(terms[cell[0]][hit])


# ---------------------------------------------------------------------------------------------------------------------
# poses: a set of dimers, nucleotides 2 k and 2 k + 1
# ---------------------------------------------------------------------------------------------------------------------
class Poses:
    """``center`` (2 n, 3), ``quat`` (2 n, 4), ``seq`` (2 n,), ``is_end`` (2 n,), ``bonded`` (n,) bool, ``cell`` (n,) int
    (index into ``cells``; -1: the aligned family)."""

    def __init__(self, model, center, quat, seq, is_end, bonded, cell=None, cells=()):
        self.model = model
        self.center, self.quat = np.ascontiguousarray(center, np.float64), np.ascontiguousarray(quat, np.float64)
        self.seq, self.is_end = np.asarray(seq, np.int64), np.asarray(is_end, np.int64)
        self.bonded = np.asarray(bonded, bool)
        self.n = len(self.bonded)
        self.cell = np.full(self.n, -1, np.int64) if cell is None else np.asarray(cell, np.int64)
        self.cells = list(cells)

    def pairs(self, bonded: bool) -> np.ndarray:
        k = np.nonzero(self.bonded == bonded)[0]
        return np.stack([2 * k, 2 * k + 1], 1).astype(np.int64)

    def subset(self, idx):
        idx = np.asarray(idx)
        nuc = np.stack([2 * idx, 2 * idx + 1], 1).reshape(-1)
        return Poses(self.model, self.center[nuc], self.quat[nuc], self.seq[nuc], self.is_end[nuc], self.bonded[idx], self.cell[idx],
                     self.cells)

    def tensors(self):
        return (torch.as_tensor(self.seq), torch.as_tensor(self.is_end), torch.as_tensor(self.pairs(True)),
                torch.as_tensor(self.pairs(False)))

    def per_pose(self, bonded_values, unbonded_values):
        """(n,) from per-bonded-pair and per-unbonded-pair values."""
        out = np.zeros(self.n, dtype=np.asarray(bonded_values).dtype)
        out[self.bonded] = bonded_values
        out[~self.bonded] = unbonded_values
        return out


def evaluate(poses: Poses, mutate=None, with_forces=False):
    """Oracle evaluation under the recorder -> (terms: name -> (n,) energy of every pose, masks: cell -> (n,) bool,
    intervals, [force: (n,) the forces of the terms on nucleotide j summed in magnitude, own: cell -> (n,) what that branch of that factor contributes to the
    energy of the pose, in magnitude])."""
    model, P = poses.model, params(poses.model)
    c = torch.as_tensor(poses.center).clone().requires_grad_(with_forces)
    with Recorder(mutate, probe=with_forces) as rec:
        bt, ut = orc.pair_terms(model, P, c, torch.as_tensor(poses.quat), *poses.tensors())
    terms = {}
    for name, v in {**bt, **ut}.items():
        is_b = name in BONDED_TERMS
        terms[name] = poses.per_pose(v.detach().numpy(), 0.0) if is_b else poses.per_pose(0.0, v.detach().numpy())

    def spread(cell, values, fill):
        return poses.per_pose(values, fill) if cell[0] in BONDED_TERMS else poses.per_pose(fill, values)

    masks = {cell: spread(cell, m.numpy(), False) for cell, m in rec.masks.items()}
    if not with_forces:
        return terms, masks, rec.intervals
    cells = list(rec.probes)
    force = np.zeros(poses.n)  # the forces of the terms on nucleotide j, summed in magnitude: no credit for a cancellation
    for v in {**bt, **ut}.values():
        g = torch.autograd.grad(v.sum(), c, retain_graph=True, allow_unused=True)[0]
        if g is not None:
            force += np.linalg.norm(g.numpy()[1::2], axis=1)
    total = sum(v.sum() for v in {**bt, **ut}.values())
    g = torch.autograd.grad(total, [rec.probes[k] for k in cells], allow_unused=True)
    own = {k: spread(k, np.zeros(len(rec.probes[k])) if gk is None else np.abs(gk.numpy()), 0.0) for k, gk in zip(cells, g)}
    return terms, masks, rec.intervals, force, own


def live_mask(terms, masks, cell):
    return masks[cell] & (np.abs(terms[cell[0]]) > LIVE)


def eligible(terms):
    total = sum(terms.values())
    return np.isfinite(total) & (terms["bonded_excluded_volume"] < EXC_MAX) & (terms["unbonded_excluded_volume"] < EXC_MAX)


# ---- the draws -------------------------------------------------------------------------------------------------------
def _qmul(a, b):
    a0, a1, a2, a3 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    b0, b1, b2, b3 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                     a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], 1)


def _rotor(axis, angle):
    axis = axis / np.linalg.norm(axis, axis=1, keepdims=True)
    return np.concatenate([np.cos(0.5 * angle)[:, None], np.sin(0.5 * angle)[:, None] * axis], 1)


def _unit(rng, m, d=3):
    v = rng.standard_normal((m, d))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _log_uniform(rng, lo, hi, m):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), m))


def _axes(q):
    return tuple(a.numpy() for a in orc.quat_to_axes(torch.as_tensor(q)))


def seeds(model: int):
    """The ideal geometry of every term: (name, centre_i, quat_i, centre_j, quat_j, bonded, aligned axis of j) - a
    Watson-Crick pair, the cross-stacked pair on either side (both orders), a stacked bonded neighbour, and the same
    neighbour as an unbonded pair for the coaxial term.  oxDNA: generators.ideal_duplex; oxRNA2: the first frame of the
    reference's A-form helix (an ideal B-duplex is outside the FENE well of the RNA geometry)."""
    if model == 3:
        top, traj, _, _ = H.load_golden(3, "simple-helix-12bp")
        c, q, n = traj.center[0], traj.quaternions[0], top.n_nucleotides // 2
    else:
        top, c, q = generators.ideal_duplex(12, model=model, seed=1)
        n = 12
    k = 5
    mate = lambda i: 2 * n - 1 - i  # noqa: E731
    out = []
    for name, i, j, bonded, axis in (("wc", k, mate(k), False, 0), ("wc_r", mate(k), k, False, 0),
                                      ("cross_up", k, mate(k + 1), False, 0), ("cross_up_r", mate(k + 1), k, False, 0),
                                      ("cross_down", k, mate(k - 1), False, 0), ("cross_down_r", mate(k - 1), k, False, 0),
                                      ("stacked", k, k + 1, True, 2), ("coax", k, k + 1, False, 2), ("coax_r", k + 1, k, False, 2)):
        out.append((name, c[i] - c[i], q[i], c[j] - c[i], q[j], bonded, axis))
    return out


def _candidates(model: int, seed: int, n_seed: int, n_uniform: int, theta1_only: bool = False) -> Poses:
    """The pool of draws.  ``theta1_only``: family (d) alone, the draws aimed at theta1 near pi (the checks of FP32_BLIND)."""
    rng = np.random.default_rng(1000 * model + seed)
    P = params(model)
    C, Q, B, family_d = [], [], [], []

    def add(ci, qi, cj, qj, bonded):
        m = len(cj)
        C.append(np.stack([np.broadcast_to(ci, (m, 3)), cj], 1).reshape(-1, 3))
        Q.append(np.stack([np.broadcast_to(qi, (m, 4)), qj], 1).reshape(-1, 4))
        B.append(np.full(m, bonded))

    for _, ci, qi, cj, qj, bonded, _ in seeds(model):  # rotate j about a random axis through its centre, then move it
        rot = _rotor(_unit(rng, n_seed), _log_uniform(rng, 0.02, 1.2, n_seed))
        add(ci, qi, cj + _unit(rng, n_seed) * _log_uniform(rng, 0.02, 0.7, n_seed)[:, None], _qmul(rot, np.broadcast_to(qj, (n_seed, 4))),
            bonded)

    def back_offset(q):
        a1, a2, a3 = orc.quat_to_axes(torch.as_tensor(q))
        return orc.Sites(model, P["geometry"], torch.zeros(len(q), 3, dtype=torch.float64), a1, a2, a3).back.numpy()

    # uniform relative poses, as tests/helpers.py random_dimers draws them; the bonded ones also beyond the FENE well
    m = n_uniform
    qi, qj = _unit(rng, m, 4), _unit(rng, m, 4)
    add(np.zeros(3), qi[0], _unit(rng, m) * rng.uniform(0.3, 1.2, (m, 1)), qj, False)
    Q[-1][0::2] = qi
    r0, delta = float(P["fene"]["r0_backbone"]), float(P["fene"]["delta_backbone"])
    qi, qj = _unit(rng, m, 4), _unit(rng, m, 4)
    add(np.zeros(3), qi[0], back_offset(qi) - back_offset(qj) + _unit(rng, m) * (r0 + rng.uniform(-1.3, 1.3, (m, 1)) * delta), qj, True)
    Q[-1][0::2] = qi
    # stacked seed pulled along its backbone: beyond xmax of the smoothed FENE with the stacking term still alive
    _, ci, qi, cj, qj, _, _ = seeds(model)[6]
    mm = n_seed // 4
    bi, bj = back_offset(qi[None])[0], back_offset(qj[None])[0]
    d = (cj + bj - bi) / np.linalg.norm(cj + bj - bi)
    add(ci, qi, cj + d * rng.uniform(-1.2, 1.2, (mm, 1)) * delta + 0.03 * rng.standard_normal((mm, 3)),
        _qmul(_rotor(_unit(rng, mm), _log_uniform(rng, 0.02, 0.3, mm)), np.broadcast_to(qj, (mm, 4))), True)
    # directed draws for the cells random perturbations of j alone seldom reach
    def site(q, c, name):
        a1, a2, a3 = orc.quat_to_axes(torch.as_tensor(q[None]))
        return getattr(orc.Sites(model, P["geometry"], torch.as_tensor(c[None]), a1, a2, a3), name).numpy()[0]

    def turned(c, q, pivot, axis, angle):  # a nucleotide turned about an axis through a pivot: (m, 3), (m, 4)
        rot = _rotor(np.broadcast_to(axis, (len(angle), 3)), angle)
        R = np.stack(_axes(rot), 2)
        return pivot + np.einsum("mab,b->ma", R, c - pivot), _qmul(rot, np.broadcast_to(q, (len(angle), 4)))

    def jitter(c, q, amax, tmax):
        m = len(c)
        return (c + _unit(rng, m) * _log_uniform(rng, 0.02, tmax, m)[:, None], _qmul(_rotor(_unit(rng, m), _log_uniform(rng, 0.02, amax, m)), q))

    mm = n_seed // 2
    s5, s3 = ("stack5", "stack3") if model == 3 else ("stack", "stack")
    # (a) stacked pair, one nucleotide turned about its a3 through its stacking site: the stacking distance and theta4..6 stay,
    #     the backbone site swings round - cos(phi1), cos(phi2) leave the plateau of f5
    ci_t, qi_t = turned(ci, qi, site(qi, ci, s5), _axes(qi[None])[2][0], rng.uniform(-PI, PI, mm))
    cj_t, qj_t = jitter(np.broadcast_to(cj, (mm, 3)), np.broadcast_to(qj, (mm, 4)), 0.3, 0.15)
    C.append(np.stack([ci_t, cj_t], 1).reshape(-1, 3)), Q.append(np.stack([qi_t, qj_t], 1).reshape(-1, 4)), B.append(np.full(mm, True))
    cj_t, qj_t = jitter(*turned(cj, qj, site(qj, cj, s3), _axes(qj[None])[2][0], rng.uniform(-PI, PI, mm)), 0.3, 0.15)
    add(ci, qi, cj_t, qj_t, True)
    for _, ci, qi, cj, qj, _, _ in seeds(model)[7:9]:
        # (b) coaxial pair twisted about a3 through the stacking site: theta1 up to pi (the f6 / mirrored f4 of theta1)
        add(ci, qi, *jitter(*turned(cj, qj, site(qj, cj, "stack"), _axes(qj[None])[2][0], rng.uniform(-1.6, 1.6, mm)), 0.2, 0.1), False)
        # (c) and pushed together along the line of the stacking sites: the low tail of its f2
        dr = site(qj, cj, "stack") - site(qi, ci, "stack")
        r = np.linalg.norm(dr)
        add(ci, qi, *jitter(cj + (dr / r) * (rng.uniform(0.1, 0.4, (mm, 1)) - r), np.broadcast_to(qj, (mm, 4)), 0.3, 0.05), False)
        # (d) a1 of the two within 0.2 rad of parallel (theta1 near pi: f6 of oxDNA2, the f4 of 2 pi - theta1 of oxDNA1), pulled
        #     apart to where the backbone sites clear each other, tilted about a1 (oxDNA2's backbone site is off the a1 line)
        md = 2 * n_seed
        (a1i, _, a3i), (a1j, _, a3j) = (tuple(a[0] for a in _axes(q[None])) for q in (qi, qj))
        twist = np.arctan2(np.dot(np.cross(a1j, a1i), a3j), np.dot(a1j, a1i))
        c_t, q_t = turned(cj, qj, site(qj, cj, "stack"), a3j, twist + rng.uniform(-0.2, 0.2, md))
        a1t = _axes(q_t)[0]
        tilt = _rotor(a1t, rng.uniform(-0.9, 0.9, md))
        pivot = c_t + float(P["geometry"]["pos_stack" if model == 3 else "com_to_stacking"]) * a1t
        c_t = pivot + np.einsum("mab,mb->ma", np.stack(_axes(tilt), 2), c_t - pivot)
        c_t = c_t + (dr / r) * (rng.uniform(0.45, 0.63, (md, 1)) - r) + 0.04 * rng.standard_normal((md, 3))
        add(ci, qi, c_t, _qmul(tilt, q_t), False)
        family_d.append(len(C) - 1)
    if model != 1:  # Debye-Hueckel: backbone sites either side of r_high, out to the cut-off
        mm = n_seed // 2
        qi, qj = _unit(rng, mm, 4), _unit(rng, mm, 4)
        rh, rc = float(P["debye"]["r_high"]), float(P["debye"]["r_cut"])
        r = np.where(rng.random(mm) < 0.5, rng.uniform(0.5 * rh, rc, mm), rh + rng.uniform(-0.1, 0.1, mm) * (rc - rh))
        add(np.zeros(3), qi[0], back_offset(qi) - back_offset(qj) + _unit(rng, mm) * r[:, None], qj, False)
        Q[-1][0::2] = qi
    if theta1_only:
        C, Q, B = ([X[k] for k in family_d] for X in (C, Q, B))
    center, quat, bonded = np.concatenate(C), np.concatenate(Q), np.concatenate(B)
    n = len(bonded)
    seq = rng.integers(0, 4, 2 * n)
    wc = rng.random(n) < 0.75  # hydrogen bonds need Watson-Crick partners
    seq[1::2] = np.where(wc, 3 - seq[0::2], seq[1::2])
    is_end = rng.integers(0, 2, 2 * n)  # end and non-end nucleotides: whole and half charges
    # fp32-representable relative poses (the grid offset is added, and the sum rounded again, when the set is laid out)
    return Poses(model, center.astype(np.float32).astype(np.float64), quat.astype(np.float32).astype(np.float64), seq, is_end, bonded)


def aligned_family(model: int) -> Poses:
    """The unperturbed seeds with nucleotide j turned about the axis the pair shares (a1 of a Watson-Crick or cross-stacked
    pair, a3 of a stacked one): the cosines of the aligned axes stay +-1 to rounding - the edge of the clamped acos."""
    C, Q, B = [], [], []
    for name, ci, qi, cj, qj, bonded, axis in seeds(model):
        if name.endswith("_r"):
            continue
        if model == 3 and name == "coax":
            # oxRNA2's coaxial term has theta0_coax_4 = 0.151: at theta4 = 0 its f4 is a cone in the orientation, the torque has
            # no value there (central differences of the oracle's energy and its autograd disagree by 20 %) - nothing to compare
            continue
        if not name.startswith("cross"):  # the shared axis made exactly (anti)parallel first (the oxRNA2 seeds are a thermal frame)
            ai, aj = _axes(qi[None])[axis][0], _axes(qj[None])[axis][0]
            target = ai * np.sign(np.dot(ai, aj))
            v = np.cross(aj, target)
            if np.linalg.norm(v) > 1e-14:
                qj = _qmul(_rotor(v[None], np.array([np.arctan2(np.linalg.norm(v), np.dot(aj, target))])), qj[None])[0]
        ax = _axes(qj[None])[axis][0]
        base = cj + float(params(model)["geometry"]["pos_base" if model == 3 else "com_to_hb"]) * _axes(qj[None])[0][0]
        for ang in (0.0, 0.05, -0.11, 0.3):
            rot = _rotor(ax[None], np.array([ang]))
            pivot = base if axis == 0 else cj  # about the line of a1 through the base site / about a3 through the centre
            R = np.stack(_axes(rot), 2)[0]  # columns: the images of e_x, e_y, e_z
            C += [ci, pivot + R @ (cj - pivot)]
            Q += [qi, _qmul(rot, qj[None])[0]]
            B.append(bonded)
    n = len(B)
    seq = np.tile([0, 3], n)
    c32 = np.array(C).astype(np.float32).astype(np.float64)
    return Poses(model, c32, np.array(Q).astype(np.float32).astype(np.float64), seq, np.tile([1, 0], n), np.array(B))


def lay_out(poses: Poses) -> Poses:
    """The dimers on a cubic grid of 8 units, centres rounded to fp32 once more (both precisions see the same numbers)."""
    side = int(np.ceil(poses.n ** (1.0 / 3.0)))
    k = np.arange(poses.n)
    grid = np.stack([k % side, (k // side) % side, k // (side * side)], 1) * GRID
    c = (poses.center + np.repeat(grid, 2, axis=0)).astype(np.float32).astype(np.float64)
    return Poses(poses.model, c, poses.quat, poses.seq, poses.is_end, poses.bonded, poses.cell, poses.cells)


def mutation_ratio(poses: Poses, cell):
    """Per pose: by how much a 1 % error in ``cell`` moves the force or the body torque on either nucleotide, in units of
    1e-3 of that nucleotide's own largest component - the part of the fp32 bound no other pose of a set can add to.  Above
    1 the fp32 comparison can show the error (it does once the rms of the set the pose is judged in is small enough); below
    1 it cannot, whatever else is in the set."""
    _, gc0, gq0 = oracle_energy(poses)
    _, gc1, gq1 = oracle_energy(poses, mutate=cell)
    t0, t1 = body_torque(poses.quat, gq0), body_torque(poses.quat, gq1)
    tiny = 1e-300
    rf = np.abs(gc1 - gc0).max(1) / (1e-3 * np.abs(gc0).max(1) + tiny)
    rt = np.abs(t1 - t0).max(1) / (1e-3 * np.abs(t0).max(1) + tiny)
    return np.maximum(rf, rt).reshape(-1, 2).max(1)


def reference_spread(poses: Poses, seed: int = 0, trials: int = 2):
    """Per pose: how far the ORACLE's forces and body torques move when every input coordinate moves by one part in 2^24 (an
    fp32 rounding), in units of the nucleotide's own largest component - the conditioning of the pose.  Terms that cancel
    (a Debye repulsion against a coaxial tail, say) make poses no single-precision evaluation can hold to 1e-3."""
    rng = np.random.default_rng(seed)
    _, gc0, gq0 = oracle_energy(poses)
    t0 = body_torque(poses.quat, gq0)
    worst = np.zeros(poses.n)
    for _ in range(trials):
        c = poses.center * (1.0 + 2.0**-24 * rng.choice([-1.0, 1.0], poses.center.shape))
        q = poses.quat * (1.0 + 2.0**-24 * rng.choice([-1.0, 1.0], poses.quat.shape))
        _, gc, gq = oracle_energy(poses, c, q)
        t = body_torque(q, gq)
        rel = np.maximum(np.abs(gc - gc0).max(1) / (np.abs(gc0).max(1) + 1e-300), np.abs(t - t0).max(1) / (np.abs(t0).max(1) + 1e-300))
        worst = np.maximum(worst, rel.reshape(-1, 2).max(1))
    return worst


MAX_SPREAD = 3e-5  # poses whose reference moves by more under one fp32 rounding of the inputs are not selected: 1/30 of 1e-3
K_SHORTLIST = 256  # poses per cell that go on to the second stage of the selection


def build_poses(model: int, n_seed: int = 40_000, n_uniform: int = 100_000, seed: int = 0, chunk: int = 50_000) -> Poses:
    """Draw, evaluate, select.  Per reachable cell, among the eligible live poses in that branch: first the K_SHORTLIST
    where the cell's own branch carries the largest share - its contribution to the energy of the pair over the forces of
    all terms on the pair; of those, without the ill-conditioned ones (reference_spread above MAX_SPREAD), the K_SELECT where
    a 1 % error in the cell moves the forces most (mutation_ratio), each pose owned by one cell.  Then the aligned family;
    laid out on the grid."""
    cand = _candidates(model, seed, n_seed, n_uniform)
    best: dict = {}
    intervals = {}
    for lo in range(0, cand.n, chunk):
        idx = np.arange(lo, min(lo + chunk, cand.n))
        terms, masks, iv, force, own = evaluate(cand.subset(idx), with_forces=True)
        intervals.update(iv)
        ok = eligible(terms)
        for cell, m in masks.items():
            hit = np.nonzero(m & ok & (np.abs(terms[cell[0]]) > LIVE))[0]
            share = own[cell][hit] / (force[hit] + 1e-12)
            top = np.argsort(-share, kind="stable")[:K_SHORTLIST]
            best.setdefault(cell, []).extend(zip(-share[top], idx[hit][top]))
    cells = reachable_cells(intervals)
    chosen, owner = [], []
    for ci, cell in enumerate(cells):
        short = np.array([i for _, i in sorted(best.get(cell, []))[:K_SHORTLIST]], dtype=np.int64)
        if len(short):
            short = short[reference_spread(cand.subset(short)) <= MAX_SPREAD]
        if not len(short):
            continue
        ratio = mutation_ratio(cand.subset(short), cell)
        taken = 0
        for k in np.argsort(-ratio, kind="stable"):
            i = short[k]
            # (beyond the K_LIVE the coverage needs, only poses that add to the sensitivity: a pose with large forces and a
            #  small ratio would only raise the rms its cell is judged with)
            if taken < K_SELECT and (taken < K_LIVE or ratio[k] > 2.0) and int(i) not in chosen:
                chosen.append(int(i))
                owner.append(ci)
                taken += 1
    sel = cand.subset(np.array(chosen, dtype=np.int64))
    sel.cell, sel.cells = np.array(owner), cells
    al = aligned_family(model)
    both = Poses(model, np.concatenate([sel.center, al.center]), np.concatenate([sel.quat, al.quat]), np.concatenate([sel.seq, al.seq]),
                 np.concatenate([sel.is_end, al.is_end]), np.concatenate([sel.bonded, al.bonded]),
                 np.concatenate([sel.cell, al.cell]), cells)
    return lay_out(both)


def cell_table(poses: Poses):
    """-> (rows of (cell, live poses, waiver reason or None) for every reachable cell, the text of the table)."""
    terms, masks, intervals = evaluate(poses)
    ok = eligible(terms)
    rows = []
    for cell in reachable_cells(intervals):
        rows.append((cell, int((live_mask(terms, masks, cell) & ok).sum()), WAIVERS.get((poses.model, *cell))))
    text = "\n".join(f"model {poses.model} {c[0]:26s} {c[1]:7s} {c[2]:10s} live {n:4d}{'  WAIVED: ' + w if w else ''}" for c, n, w in rows)
    return rows, text


# ---- the fixture -----------------------------------------------------------------------------------------------------
def fixture_path(model: int):
    return FIXTURE_DIR / f"model{model}.dat"


def fixture_text(poses: Poses) -> str:
    lines = [f"# oxDNA branch poses, model {poses.model}: one dimer per row (tests/golden/make_branch_poses.py)",
             "# centre_i(3) quat_i(4) centre_j(3) quat_j(4) base_i base_j bonded end_i end_j cell"]
    lines += [f"# cell {k} {t} {f} {b}" for k, (t, f, b) in enumerate(poses.cells)]
    for k in range(poses.n):
        i, j = 2 * k, 2 * k + 1
        nums = [*poses.center[i], *poses.quat[i], *poses.center[j], *poses.quat[j]]
        lines.append(" ".join("%.9g" % v for v in nums)
                     + f" {poses.seq[i]} {poses.seq[j]} {int(poses.bonded[k])} {poses.is_end[i]} {poses.is_end[j]} {poses.cell[k]}")
    return "\n".join(lines) + "\n"


@functools.lru_cache(maxsize=None)
def load_fixture(model: int) -> Poses:
    cells, rows = [], []
    for line in fixture_path(model).read_text().splitlines():
        if line.startswith("# cell "):
            _, _, _, t, f, b = line.split()
            cells.append((t, f, b))
        elif not line.startswith("#"):
            rows.append(line.split())
    a = np.array([[float(x) for x in r[:14]] for r in rows])
    i = np.array([[int(x) for x in r[14:]] for r in rows])
    center = np.stack([a[:, 0:3], a[:, 7:10]], 1).reshape(-1, 3)
    quat = np.stack([a[:, 3:7], a[:, 10:14]], 1).reshape(-1, 4)
    return Poses(model, center, quat, i[:, 0:2].reshape(-1), i[:, 3:5].reshape(-1), i[:, 2] != 0, i[:, 5], cells)


# ---------------------------------------------------------------------------------------------------------------------
# the comparisons (kernel or mutated oracle against the plain oracle)
# ---------------------------------------------------------------------------------------------------------------------
TOL = {"fp64": 1e-9, "fp32": 1e-3}
DT = 0.005
INERTIA = np.array([1.0, 1.0, 1.0])


def body_torque(q, gq):
    return orc.quat_grad_to_body_torque(torch.as_tensor(q), torch.as_tensor(gq)).numpy()


def oracle_energy(poses: Poses, center=None, quat=None, mutate=None):
    """-> (terms (8,), dU/dcentre, dU/dquat) of the whole set by autograd."""
    c = torch.as_tensor(poses.center if center is None else center).clone().requires_grad_(True)
    q = torch.as_tensor(poses.quat if quat is None else quat).clone().requires_grad_(True)
    with Recorder(mutate):
        e = orc.energy_terms(poses.model, params(poses.model), c, q, *poses.tensors())
    gc, gq = torch.autograd.grad(e.sum(), (c, q))
    e = e.detach().numpy()
    return np.concatenate([e, np.zeros(8 - len(e))]), gc.numpy(), gq.numpy()


def oracle_step(poses: Poses, mutate=None):
    """One frictionless step from rest, as tests/test_gpu_md_at_size.py builds it: oracle forces and torques, then
    oracle/langevin_oracle.py's drift.  -> (momenta, angular momenta, term energies at the stepped state)."""
    qn = poses.quat / np.linalg.norm(poses.quat, axis=1, keepdims=True)  # the step kernel normalises on entry

    def forces(x, q):
        e, gc, gq = oracle_energy(poses, x, q, mutate)
        return e, -gc, body_torque(q, gq)

    _, F0, t0 = forces(poses.center, qn)
    p, L = 0.5 * DT * F0, 0.5 * DT * t0
    x, q, L = drift(poses.center, qn, p, L, 0.5 * DT, 1.0, INERTIA)
    x, q, L = drift(x, q, p, L, 0.5 * DT, 1.0, INERTIA)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    e1, F1, t1 = forces(x, q)
    return p + 0.5 * DT * F1, L + 0.5 * DT * t1, e1


def _cells_of(poses: Poses, rows):
    """Name the cells the nucleotides ``rows`` belong to."""
    ids = sorted({int(poses.cell[r // 2]) for r in rows})
    return [("aligned",) if k < 0 else poses.cells[k] for k in ids]


def _live_cells_of(poses: Poses, pose: int):
    """Every cell the pose lies in with a live term (a pose is owned by one cell and lies in many); evaluated once per set."""
    if not hasattr(poses, "_live_cells"):
        terms, masks, _ = evaluate(poses)
        poses._live_cells = {cell: live_mask(terms, masks, cell) for cell in masks}
    return [cell for cell, m in poses._live_cells.items() if m[pose]]


def compare_energies(poses, got, ref, precision) -> list:
    """The eight term energies: fp64 1e-9, fp32 1e-3, of the largest term."""
    tol = TOL[precision] * np.abs(ref).max()
    bad = np.nonzero(np.abs(got - ref) > tol)[0]
    return [f"energy of {H.SPLIT_COLUMNS[1 + k]}: got {got[k]!r}, want {ref[k]!r} (tolerance {tol:.3g})" for k in bad]


def compare_vectors(poses, got, ref, precision, what, fp64_scale="rms") -> list:
    """A vector per nucleotide (force, torque, dU/dquat, momentum).  fp64: 1e-9 of the rms over the set for the gradients (as
    tests/test_gpu_oxdna_energy.py::test_random_dimers), 1e-9 max(1, largest component) for the momenta of a step; fp32:
    per nucleotide 1e-3 of (its own largest component + the rms over the set) - over the whole set, and over the poses of
    every cell taken as a set of their own (a cell of weak tails is not hidden behind the excluded-volume contacts of the
    rest: single-precision error scales with the terms of the pair, not with other dimers)."""
    err, own = np.abs(got - ref).max(1), np.abs(ref).max(1)
    if precision == "fp64":
        allowed = np.full(len(ref), 1e-9 * (np.sqrt((ref**2).mean()) if fp64_scale == "rms" else max(1.0, np.abs(ref).max())))
    else:
        allowed = 1e-3 * (own + np.sqrt((ref**2).mean()))
        group = np.repeat(poses.cell, 2)
        for k in np.unique(group):
            rows = group == k
            allowed[rows] = np.minimum(allowed[rows], 1e-3 * (own[rows] + np.sqrt((ref[rows] ** 2).mean())))
    bad = np.nonzero(~(err <= allowed))[0]
    out = []
    for k in sorted({int(poses.cell[r // 2]) for r in bad}):  # one line per cell that owns an offending pose
        rows = bad[poses.cell[bad // 2] == k]
        w = rows[np.argmax(err[rows] / allowed[rows])]
        out.append(f"{what}, cell {_cells_of(poses, [w])[0]}: {len(rows)} nucleotides off; worst pose {w // 2}: got {got[w]}, want {ref[w]}, "
                   f"allowed {allowed[w]:.3g}; that pose has a live term in {_live_cells_of(poses, w // 2)}")
    return out


def compare_gradients(poses, got_gc, got_gq, ref_gc, ref_gq, precision) -> list:
    """dU/dcentre and dU/dquat.  The component of dU/dquat along q moves nothing and is not comparable where a cosine sits on
    the clamp (tests/test_gpu_md_at_size.py::test_12kbp_two_fp64_steps_and_forces_match_the_oracle_directly): fp32 compares the
    body torque only; fp64 the body torque everywhere and the raw gradient outside the aligned family."""
    out = compare_vectors(poses, got_gc, ref_gc, precision, "dU/dcentre")
    out += compare_vectors(poses, body_torque(poses.quat, got_gq), body_torque(poses.quat, ref_gq), precision, "body torque")
    if precision == "fp64":
        free = np.repeat(poses.cell >= 0, 2)
        sub = poses.subset(np.nonzero(poses.cell >= 0)[0])
        out += compare_vectors(sub, got_gq[free], ref_gq[free], precision, "dU/dquat")
    return out


def compare_param_grads(keys, got, ref) -> list:
    """dU/dtheta of every leaf: 1e-6 max(|ref|, 1e-3 max |ref|)."""
    bad = np.nonzero(np.abs(got - ref) > 1e-6 * np.maximum(np.abs(ref), 1e-3 * np.abs(ref).max()))[0]
    return [f"dU/d{keys[i]}: got {got[i]!r}, want {ref[i]!r}" for i in bad]


def compare_step(poses, got_p, got_L, got_e, ref_p, ref_L, ref_e, precision) -> list:
    out = compare_vectors(poses, got_p, ref_p, precision, "momentum", "max")
    out += compare_vectors(poses, got_L, ref_L, precision, "angular momentum", "max")
    return out + compare_energies(poses, got_e, ref_e, precision)


def leaf_cfg(model: int):
    """The configuration with every independent parameter a leaf (tests/test_gpu_oxdna_energy.py::_leaf_cfg)."""
    from mythos_amd.input import defaults

    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    leaves = {}
    for sec, d in cfg.items():
        if sec == "geometry":
            continue
        for k, v in d.items():
            t = torch.tensor(float(v), dtype=torch.float64, requires_grad=True)
            d[k] = t
            leaves[(sec, k)] = t
    return sim, cfg, leaves


def oracle_param_grads(poses: Poses, mutate=None):
    """-> (keys, dU/dleaf) by autograd through the oracle's own init_params."""
    sim, cfg, leaves = leaf_cfg(poses.model)
    P = orc.init_all(poses.model, cfg, kt=sim["kT"], salt_conc=SALT[poses.model], half_charged_ends=HCE[poses.model])
    with Recorder(mutate):
        u = orc.energy(poses.model, P, torch.as_tensor(poses.center), torch.as_tensor(poses.quat), *poses.tensors())
    keys = list(leaves)
    g = torch.autograd.grad(u, [leaves[k] for k in keys], allow_unused=True)
    return keys, np.array([0.0 if x is None else float(x) for x in g])
