"""Shared by tests/test_martini_restraints_cpu.py and tests/test_gpu_martini_restraints.py: the restraint sets on the
257-bead synthetic system and on free beads, a NumPy transcription of what the kernels do with the LOWERED arrays (so the
lowering is checked on the CPU against tests/martini_restraints_ref.py, which never sees those arrays), and the oracle of
the Langevin step with the reference field added."""

from __future__ import annotations

import functools

import numpy as np

from mythos_amd.simulators.martini_restraints import (FlatBottomRestraint, MartiniRestraints, PositionRestraint, PullCoordinate,
                                                       PullGroup)
from tests import martini_restraints_ref as REF
from tests import martini_synth as S

KB = 0.0083144626
DT = 0.01
N_REP = 3
HUB = 7  # the bead of the full set with a position restraint, two flat-bottom terms and membership in two coordinates


def lowered_field(a, x, masses, s, dt, rep):
    """(F, energies (4,), xi) of replica ``rep`` from the arrays of ``MartiniRestraints.lower``: the flags, the parameter
    rows and the group ranges read the way csrc/martini_restraints.h reads them."""
    x = np.asarray(x, dtype=np.float64)
    F, e = np.zeros_like(x), np.zeros(4)
    box = None if a["boxes"] is None else a["boxes"][rep]
    for t, i in enumerate(a["pr_index"]):
        d = x[i] - a["pr_ref"][rep, t]
        F[i] -= a["pr_k"][t] * d
        e[0] += 0.5 * (a["pr_k"][t] * d * d).sum()
    for t, i in enumerate(a["fb_index"]):
        f = int(a["fb_flags"][t])
        shape, axis, invert = f & 3, (f >> 2) & 3, (f >> 4) & 1
        k, r = a["fb_param"][rep, t, :2]
        rho = x[i] - a["fb_param"][rep, t, 2:5]
        if shape == 1:
            rho[axis] = 0.0
        if shape == 2:
            rho = rho * (np.arange(3) == axis)
        d = np.sqrt(rho @ rho)
        if (d < r) if invert else (d > r):
            e[1] += 0.5 * k * (d - r) ** 2
            if d > 0:
                F[i] -= k * (d - r) * rho / d
    com, mass = [], []
    for g in range(len(a["g_pbc_ref"])):
        mem = a["g_member"][a["g_first"][g]:a["g_first"][g + 1]]
        y = x[mem]
        if a["g_pbc_ref"][g] >= 0:
            ref = x[a["g_pbc_ref"][g]]
            y = ref + (y - ref) - box * np.round((y - ref) / box)
        com.append((masses[mem][:, None] * y).sum(0) / masses[mem].sum())
        mass.append(masses[mem].sum())
    xi = np.zeros(len(a["p_flags"]))
    for p, f in enumerate(a["p_flags"]):
        f = int(f)
        A, B = a["p_groups"][p]
        q = a["p_param"][rep, p]
        D = com[B] - (com[A] if A >= 0 else q[6:9])
        if f & 4:
            D = D - box * np.round(D / box)
        if f & 2:
            xi[p], ev = D @ q[3:6], q[3:6]
        else:
            D = D * np.array([(f >> (4 + ax)) & 1 for ax in range(3)])
            xi[p] = np.sqrt(D @ D)
            ev = D / xi[p] if xi[p] > 0 else np.zeros(3)
        if f & 1:
            u, du = q[0] * xi[p], q[0]
        else:
            dev = xi[p] - q[1] - q[2] * s * dt
            u, du = 0.5 * q[0] * dev * dev, q[0] * dev
        e[3 if f & 1 else 2] += u
        for side, g in ((0, A), (1, B)):
            if g < 0:
                continue
            mem = a["g_member"][a["g_first"][g]:a["g_first"][g + 1]]
            F[mem] += (-du if side else du) * ev[None, :] * (masses[mem] / mass[g])[:, None]
    return F, e, xi


def minimum_image_margin(rs, x, masses, box, topology=None):
    """The smallest distance, in units of the box edge, of any minimum-image argument of the set (a group member against
    its pbc_ref, a periodic D) from the half box where the image flips: the CPU check asks for a clear margin."""
    margin = 0.5
    for c in rs.pulls:
        coms = []
        for g in (c.group_a, c.group_b):
            if g is None:
                coms.append(np.asarray(c.origin, dtype=np.float64))
                continue
            mem = g.indices(topology)
            if g.pbc_ref is not None:
                fr = (x[mem] - x[g.pbc_ref]) / box
                margin = min(margin, float(np.abs(np.abs(fr - np.round(fr)) - 0.5).min()))
            coms.append(REF.group_com(x, masses, mem, box, g.pbc_ref)[0])
        if c.periodic:
            fr = (coms[1] - coms[0]) / box
            margin = min(margin, float(np.abs(np.abs(fr - np.round(fr)) - 0.5).min()))
    return margin


@functools.lru_cache(maxsize=None)
def n257():
    """The 257-bead synthetic system, wrapped into its box, for three replicas with their own boxes (enlarged by 0 - 3 %,
    positions scaled with them): dict(s, n, masses, boxes (3, 3), ref (3, 257, 3) - the state that references left None are
    taken from, every bead up to 0.03 nm per axis off pos so that no restraint sits at its minimum -, pos (3, 257, 3) - the
    state the field is evaluated at and runs start from: the synthetic system's own, whose geometry martini_synth.check vouches for)."""
    s = S.get("n257")
    box = s["box"][0]
    xw = s["pos"][0] - s["shift"] * box
    f = 1.0 + 0.03 * np.random.default_rng(23).uniform(size=(N_REP, 3))
    f[0] = 1.0
    boxes = box[None, :] * f
    pos = xw[None] * f[:, None, :]
    ref = pos + np.random.default_rng(24).uniform(-0.03, 0.03, size=pos.shape)
    return dict(s=s, n=s["n"], masses=np.asarray(s["mass"], dtype=np.float64), boxes=boxes, ref=ref, pos=pos)


def _straddling_pair(x, box):
    """Two beads within 1 nm of each other through the x face: (i on the low side, j on the high side)."""
    lo, hi = np.flatnonzero(x[:, 0] < 0.45), np.flatnonzero(x[:, 0] > box[0] - 0.45)
    for i in lo:
        d = x[hi] - x[i]
        d[:, 0] -= box[0]
        near = np.flatnonzero(np.sqrt((d * d).sum(1)) < 1.0)
        if near.size and i != HUB and hi[near[0]] != HUB:
            return int(i), int(hi[near[0]])
    raise AssertionError("no pair of beads across the x face")


@functools.lru_cache(maxsize=None)
def sets():
    """name -> MartiniRestraints on the n257 system.
      none   0 restrained beads
      one    1 restrained bead (a position restraint)
      full   257 restrained beads (the kick spans two workgroups; three replicas: four): a position restraint on every bead,
             per-axis k with zeros; flat-bottom terms of every shape, plain and inverted, inside and outside their r; four
             pull coordinates - umbrella distance over x, y between a group of 1 (HUB) and a group of 2, periodic, moving;
             umbrella direction between a group of all 257 (a member stride of 256 wraps) and a group of 3 with HUB, init and
             k per replica; constant-force direction from an absolute origin to a pair that straddles the x face (pbc_ref);
             constant-force distance between two small groups, not periodic."""
    c = n257()
    n, x, box = c["n"], c["pos"][0], c["boxes"][0]
    rng = np.random.default_rng(99)
    kk = rng.uniform(200.0, 3000.0, size=(n, 3))
    kk[::5, 1] = 0.0
    kk[3] = 0.0
    position = [PositionRestraint(index=i, k=tuple(kk[i]), reference=None if i % 2 else tuple(x[i] + rng.uniform(-0.05, 0.05, 3)))
                for i in range(n)]
    flat = [FlatBottomRestraint(index=HUB, shape="sphere", r=0.1, k=800.0, reference=tuple(x[HUB] + [0.2, -0.1, 0.15])),
            FlatBottomRestraint(index=HUB, shape="layer", axis="y", r=0.3, k=500.0, invert=True, reference=tuple(x[HUB] + [0.0, 0.1, 0.0])),
            FlatBottomRestraint(index=11, shape="cylinder", axis="z", r=0.05, k=700.0, reference=tuple(x[11] + [0.1, 0.1, 5.0])),
            FlatBottomRestraint(index=12, shape="cylinder", axis="x", r=0.5, k=700.0, invert=True, reference=tuple(x[12] + [3.0, 0.1, 0.2])),
            FlatBottomRestraint(index=13, shape="sphere", r=0.4, k=650.0, invert=True, reference=tuple(x[13] + [0.1, 0.1, 0.1])),
            FlatBottomRestraint(index=14, shape="layer", axis=0, r=0.1, k=900.0, reference=tuple(x[14] + [-0.3, 1.0, 1.0])),
            FlatBottomRestraint(index=15, shape="sphere", r=1.0, k=900.0, reference=tuple(x[15] + [0.1, 0.0, 0.0])),  # inside: no force
            FlatBottomRestraint(index=256, shape="sphere", r=0.0, k=300.0, reference=None),
            # d = 0 in replica 0 (in double): energy k r^2 / 2 and no force
            FlatBottomRestraint(index=255, shape="sphere", r=0.2, k=300.0, invert=True, reference=tuple(c["pos"][0][255]))]
    lo, hi = _straddling_pair(x, box)
    # the absolute origin 0.6 - 0.7 nm per axis off the pair's centre: D stays clear of the half box in every replica
    origin = tuple(REF.group_com(x, c["masses"], (lo, hi), box, lo)[0] - np.array([0.7, 0.6, -0.65]))
    everyone = PullGroup(members=tuple(range(n)))
    pulls = [
        PullCoordinate(group_a=PullGroup(members=(HUB,)), group_b=PullGroup(members=(20, 31)), kind="umbrella", geometry="distance",
                       dim=(True, True, False), k=1500.0, init=(0.4, 0.9, 1.3), rate=2.5e-3, periodic=True),
        PullCoordinate(group_a=everyone, group_b=PullGroup(members=(HUB, 40, 41)), kind="umbrella", geometry="direction", vec=(1.0, 2.0, -1.0),
                       k=(800.0, 1200.0, 50.0), init=(-0.2, 0.1, 0.6), rate=-1.0e-3, periodic=False),
        PullCoordinate(group_a=None, group_b=PullGroup(members=(lo, hi), pbc_ref=lo), kind="constant-force", geometry="direction",
                       vec=(0.0, 0.0, 2.0), k=-120.0, origin=origin, periodic=True),
        PullCoordinate(group_a=PullGroup(members=(50, 51)), group_b=PullGroup(members=(60,)), kind="constant-force", geometry="distance",
                       k=75.0, periodic=False),
    ]
    return dict(none=MartiniRestraints(), one=MartiniRestraints(position=[PositionRestraint(index=5, k=(1000.0, 0.0, 250.0))]),
                full=MartiniRestraints(position=position, flat_bottom=flat, pulls=pulls))


def free_beads(n, edge=6.0, seed=41):
    """n beads without interactions (epsilon = 0, no bonds) in a cubic box of ``edge`` nm: the arguments of MartiniSystem /
    MartiniLangevinOracle, and positions inside the middle half of the box."""
    z = np.zeros(0)
    ff = (np.zeros(n, dtype=np.int32), np.array([[0.47]]), np.array([[0.0]]), np.zeros((0, 2), np.int32), z, z, np.zeros((0, 3), np.int32), z, z)
    pos = edge * (0.25 + 0.5 * np.random.default_rng(seed).uniform(size=(n, 3)))
    return dict(n=n, ff=ff, box=np.full(3, edge), pos=pos, mass=np.random.default_rng(seed + 1).uniform(40.0, 90.0, size=n))


def oracle_with_field(rs, ff, use_g96, box, dt, kT, gamma, mass, seed, reference_pos, rep=0):
    """MartiniLangevinOracle whose ``forces`` add the reference field at the step count of the frame they are taken at."""
    from oracle.martini_langevin_oracle import MartiniLangevinOracle

    class WithField(MartiniLangevinOracle):
        def run(self, x, v, n_steps):
            self._s = self.step_index  # the frame of the first evaluation of a run; every later one is one step on
            return super().run(x, v, n_steps)

        def forces(self, x):
            e, F = super().forces(x)
            Fx, _, _ = REF.field(rs, x, self.mass[:, 0], self.box.numpy(), self._s, self.dt, rep, reference_pos)
            self._s += 1
            return e, F + Fx

    return WithField(*ff, use_g96, box, dt, kT, gamma, mass, seed=seed)
