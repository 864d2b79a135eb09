"""Position-dependent external forces of the oxDNA Langevin integrator (mythos_langevin_set_restraints): the three fixes
of the reference's stretch-torsion protocol (data/templates/lammps-stretch-tors/), all on centres of mass.

    SelfTether(index, k, anchor=None, axes=(1, 1, 1))    F_i = -k A (x_i - a_i) on each listed nucleotide (LAMMPS spring/self)
    SumRestraint(index, k, target=None, axes=(1, 1, 0))  F_i = -k A (sum_j x_j - s0) on every member (addforce with a variable
                                                          of the summed coordinates)
    GroupTorque(index, torque)                            F_i = (T x d_i) / S, d_i from the group's centroid (addtorque)

``anchor=None`` / ``target=None``: the positions (their sum) of the initial state - the ``reference_center`` of
``LangevinIntegrator.set_restraints``, the ``init_state`` of ``HipMDSimulator.run``.  ``Restraints.lower`` turns a set
into the flat arrays of the C ABI, once per replica.

Beside them, a set of its own (mythos_langevin_set_point_forces): oxDNA's external forces on single nucleotides -
``MovingString``, ``Trap``, ``MutualTrap``, ``RepulsionPlane``, ``RepulsionSphere`` in a ``PointForces`` - further down.
"""

from __future__ import annotations

import dataclasses as dc

import numpy as np

KIND_SUM, KIND_TORQUE = 0, 1  # enum mythos_restraint_kind of include/mythos_hip.h


def _index(index) -> tuple:
    return tuple(int(i) for i in np.asarray(index, dtype=np.int64).reshape(-1))


def _mask(axes) -> int:
    a = tuple(int(bool(x)) for x in axes)
    if len(a) != 3:
        raise ValueError(f"axes = {axes}: three 0 / 1 flags (x, y, z)")
    return a[0] | (a[1] << 1) | (a[2] << 2)


@dc.dataclass(frozen=True)
class SelfTether:
    """Each listed nucleotide is tied to its own anchor: ``anchor`` (m, 3), or None for its initial position."""

    index: tuple
    k: float
    anchor: tuple | None = None
    axes: tuple = (1, 1, 1)

    def __post_init__(self):
        object.__setattr__(self, "index", _index(self.index))
        if self.anchor is not None:
            a = np.asarray(self.anchor, dtype=np.float64).reshape(-1, 3)
            if a.shape[0] != len(self.index):
                raise ValueError(f"SelfTether: {a.shape[0]} anchors for {len(self.index)} nucleotides")
            object.__setattr__(self, "anchor", tuple(map(tuple, a.tolist())))
        object.__setattr__(self, "axes", tuple(int(bool(x)) for x in self.axes))
        _mask(self.axes)


@dc.dataclass(frozen=True)
class SumRestraint:
    """The sum of the listed positions is tied to ``target`` (3,), or None for the sum in the initial state."""

    index: tuple
    k: float
    target: tuple | None = None
    axes: tuple = (1, 1, 0)

    def __post_init__(self):
        object.__setattr__(self, "index", _index(self.index))
        if self.target is not None:
            object.__setattr__(self, "target", tuple(np.asarray(self.target, dtype=np.float64).reshape(3).tolist()))
        object.__setattr__(self, "axes", tuple(int(bool(x)) for x in self.axes))
        _mask(self.axes)


@dc.dataclass(frozen=True)
class GroupTorque:
    """Forces on the listed centres whose torque about the group's centroid is ``torque`` (3,)."""

    index: tuple
    torque: tuple

    def __post_init__(self):
        object.__setattr__(self, "index", _index(self.index))
        object.__setattr__(self, "torque", tuple(np.asarray(self.torque, dtype=np.float64).reshape(3).tolist()))


# ------------------------------------------------------------------ point forces (mythos_langevin_set_point_forces)
# oxDNA's external forces on single nucleotides, by oxDNA's definitions; s is the integrator's step count at the frame the
# force is taken at (include/mythos_hip.h, "Time"), d = dir / |dir|.
#
#     MovingString(particle, F0, rate, dir)                F = (F0 + rate s) d
#     Trap(particle, pos0, stiff, rate=0, dir=(0, 0, 0))   F = -stiff (x - pos0 - rate s d)
#     MutualTrap(particle, ref_particle, stiff, r0,        F = stiff (r - r0 - rate s) D / r on `particle` only,
#                rate=0, pbc=False)                            D = x_ref - x (minimum image with pbc), r = |D|
#     RepulsionPlane(particle, stiff, dir, position)       h = d.x + position < 0: F = -stiff h d
#     RepulsionSphere(particle, center, r0, stiff, rate=0) |x - center| > R = r0 + rate s: F = -stiff (1 - R / |rho|) rho
KIND_STRING, KIND_TRAP, KIND_MUTUAL_TRAP, KIND_PLANE, KIND_SPHERE = range(5)  # enum mythos_point_force_kind
FLAG_PBC = 1  # MYTHOS_POINT_PBC
POINT_PARAMS = 8  # doubles per term


def _vec3(v, what) -> tuple:
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.shape != (3,):
        raise ValueError(f"{what} = {v}: three components")
    return tuple(a.tolist())


def _unit(v, what) -> tuple:
    a = np.asarray(_vec3(v, what))
    norm = float(np.linalg.norm(a))
    if not norm > 0:
        raise ValueError(f"{what} = {v} is not a direction")
    return tuple((a / norm).tolist())


@dc.dataclass(frozen=True)
class MovingString:
    """A force ramp along ``dir`` (normalised here).  Its energy, -(F0 + rate s) d.(x - origin), is defined up to the
    constant the origin sets: ``lower`` moves the origin with each replica, so every replica reports its own frame's."""

    particle: int
    F0: float
    rate: float
    dir: tuple

    def __post_init__(self):
        object.__setattr__(self, "dir", _unit(self.dir, "MovingString: dir"))


@dc.dataclass(frozen=True)
class Trap:
    """A harmonic trap at ``pos0`` that moves along ``dir`` by ``rate`` per step; a resting trap needs no ``dir``."""

    particle: int
    pos0: tuple
    stiff: float
    rate: float = 0.0
    dir: tuple = (0.0, 0.0, 0.0)

    def __post_init__(self):
        object.__setattr__(self, "pos0", _vec3(self.pos0, "Trap: pos0"))
        d = _vec3(self.dir, "Trap: dir")
        object.__setattr__(self, "dir", _unit(d, "Trap: dir") if (self.rate != 0 or any(d)) else d)


@dc.dataclass(frozen=True)
class MutualTrap:
    """``particle`` is pulled towards (pushed from) ``ref_particle`` to the distance r0 + rate s; the partner feels nothing
    from this term (oxDNA pairs two of them).  ``pbc``: the minimum image of the system's box."""

    particle: int
    ref_particle: int
    stiff: float
    r0: float
    rate: float = 0.0
    pbc: bool = False


@dc.dataclass(frozen=True)
class RepulsionPlane:
    """The half space d.x + position < 0 is repulsive, harmonically in the depth."""

    particle: int
    stiff: float
    dir: tuple
    position: float

    def __post_init__(self):
        object.__setattr__(self, "dir", _unit(self.dir, "RepulsionPlane: dir"))


@dc.dataclass(frozen=True)
class RepulsionSphere:
    """The outside of the sphere of radius r0 + rate s about ``center`` is repulsive, harmonically in the distance."""

    particle: int
    center: tuple
    r0: float
    stiff: float
    rate: float = 0.0

    def __post_init__(self):
        object.__setattr__(self, "center", _vec3(self.center, "RepulsionSphere: center"))


def _point_row(t, off):
    """One term in a replica translated by ``off``: (kind, flags, the 8 doubles of its row)."""
    off = np.asarray(off, dtype=np.float64)
    if isinstance(t, MovingString):
        return KIND_STRING, 0, [t.F0, t.rate, *t.dir, *off]
    if isinstance(t, Trap):
        return KIND_TRAP, 0, [t.stiff, t.rate, *t.dir, *(np.asarray(t.pos0) + off)]
    if isinstance(t, MutualTrap):
        return KIND_MUTUAL_TRAP, FLAG_PBC if t.pbc else 0, [t.stiff, t.r0, t.rate, 0.0, 0.0, 0.0, 0.0, 0.0]
    if isinstance(t, RepulsionPlane):
        return KIND_PLANE, 0, [t.stiff, t.position - float(np.dot(t.dir, off)), *t.dir, 0.0, 0.0, 0.0]
    if isinstance(t, RepulsionSphere):
        return KIND_SPHERE, 0, [t.stiff, t.r0, t.rate, *(np.asarray(t.center) + off), 0.0, 0.0]
    raise TypeError(f"PointForces: {type(t).__name__} is not a point force")


@dc.dataclass(frozen=True)
class PointForces:
    """A set of point forces, in the order the integrator adds them on a nucleotide that several name."""

    terms: tuple = ()

    def __post_init__(self):
        object.__setattr__(self, "terms", tuple(self.terms))

    def __bool__(self) -> bool:
        return bool(self.terms)

    def lower(self, n_one: int | None = None, n_rep: int = 1, offsets=None) -> dict:
        """-> the arrays of mythos_langevin_set_point_forces (keys: the header's argument names).

        With ``n_rep`` > 1 every term is repeated per replica at ``index + r * n_one``; ``offsets`` (n_rep, 3) are the
        translations of the replicas (ReplicaLayout.place): ``pos0`` and ``center`` move by their replica's, a plane's
        ``position`` becomes ``position - d.offset``, and the origin of a moving string's energy is the replica's offset
        (the energy of a string is defined up to that constant; its force does not change)."""
        off = np.zeros((n_rep, 3)) if offsets is None else np.asarray(offsets, dtype=np.float64).reshape(n_rep, 3)
        if n_rep > 1 and n_one is None:
            raise ValueError("PointForces.lower: replicas need n_one, the nucleotides per replica")
        kind, particle, ref, flags, param = [], [], [], [], []
        for r in range(n_rep):
            base = r * (n_one or 0)
            for t in self.terms:
                k, f, row = _point_row(t, off[r])
                partner = int(t.ref_particle) if k == KIND_MUTUAL_TRAP else int(t.particle)
                for i in (int(t.particle), partner):
                    if i < 0 or (n_one is not None and i >= n_one):
                        raise ValueError(f"{type(t).__name__}: nucleotide index {i} out of range" + ("" if n_one is None else f" [0, {n_one})"))
                kind.append(k), particle.append(int(t.particle) + base), ref.append(partner + base), flags.append(f), param.append(row)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        return {"kind": i32(kind), "particle": i32(particle), "ref_particle": i32(ref), "flags": i32(flags),
                "param": np.ascontiguousarray(param, dtype=np.float64).reshape(-1, POINT_PARAMS)}


@dc.dataclass(frozen=True)
class Restraints:
    tethers: tuple = ()
    sums: tuple = ()
    torques: tuple = ()

    def __post_init__(self):
        for name in ("tethers", "sums", "torques"):
            object.__setattr__(self, name, tuple(getattr(self, name)))

    def __bool__(self) -> bool:
        return bool(self.tethers or self.sums or self.torques)

    def lower(self, reference_center=None, n_one: int | None = None, n_rep: int = 1, offsets=None) -> dict:
        """-> the arrays of mythos_langevin_set_restraints (keys: the header's argument names).

        ``reference_center`` (n_one, 3), or (n_rep, n_one, 3) for one start per replica: resolves the None anchors and
        targets.  With ``n_rep`` > 1 every term is repeated per replica at ``index + r * n_one``; ``offsets`` (n_rep, 3) are
        the translations of the replicas (ReplicaLayout.place): an anchor moves by its replica's, the target of a sum by
        its replica's times the number of members.  ``reference_center`` is in the replicas' OWN frames."""
        ref = None if reference_center is None else np.asarray(reference_center, dtype=np.float64)
        if ref is not None and ref.ndim == 2:
            ref = np.broadcast_to(ref[None], (n_rep, *ref.shape))
        off = np.zeros((n_rep, 3)) if offsets is None else np.asarray(offsets, dtype=np.float64).reshape(n_rep, 3)
        if n_rep > 1 and n_one is None:
            raise ValueError("Restraints.lower: replicas need n_one, the nucleotides per replica")

        def check(index, what):
            for i in index:
                if i < 0 or (n_one is not None and i >= n_one):
                    raise ValueError(f"{what}: nucleotide index {i} out of range" + ("" if n_one is None else f" [0, {n_one})"))

        def need_ref(what):
            if ref is None:
                raise ValueError(f"{what} takes its positions from the initial state: pass reference_center")

        t_index, t_k, t_anchor, t_mask = [], [], [], []
        g_kind, g_first, g_member, g_vec, g_target, g_mask = [], [0], [], [], [], []
        for r in range(n_rep):
            base = r * (n_one or 0)
            for t in self.tethers:
                check(t.index, "SelfTether")
                if t.anchor is None:
                    need_ref("SelfTether(anchor=None)")
                    anchor = ref[r][list(t.index)]
                else:
                    anchor = np.asarray(t.anchor, dtype=np.float64)
                for i, a in zip(t.index, anchor):
                    t_index.append(i + base), t_k.append(float(t.k)), t_anchor.append(a + off[r]), t_mask.append(_mask(t.axes))
            for s in self.sums:
                check(s.index, "SumRestraint")
                if s.target is None:
                    need_ref("SumRestraint(target=None)")
                    target = ref[r][list(s.index)].sum(axis=0)
                else:
                    target = np.asarray(s.target, dtype=np.float64)
                g_kind.append(KIND_SUM), g_member.extend(i + base for i in s.index), g_first.append(len(g_member))
                g_vec.append([float(s.k), 0.0, 0.0]), g_target.append(target + len(s.index) * off[r]), g_mask.append(_mask(s.axes))
            for q in self.torques:
                check(q.index, "GroupTorque")
                g_kind.append(KIND_TORQUE), g_member.extend(i + base for i in q.index), g_first.append(len(g_member))
                g_vec.append(list(q.torque)), g_target.append(np.zeros(3)), g_mask.append(0)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        f64 = lambda a, w: np.ascontiguousarray(a, dtype=np.float64).reshape(-1, w) if w else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
        return {"t_index": i32(t_index), "t_k": f64(t_k, 0), "t_anchor": f64(t_anchor, 3), "t_mask": i32(t_mask),
                "g_kind": i32(g_kind), "g_first": i32(g_first), "g_member": i32(g_member), "g_vec": f64(g_vec, 3),
                "g_target": f64(g_target, 3), "g_mask": i32(g_mask)}
