"""External forces of the MARTINI integrators: position restraints, flat-bottomed restraints and pulling between the
centres of mass of two groups (GROMACS' ``[ position_restraints ]`` funct 1 / 2 and its pull code), as the sets that
``MartiniLangevinIntegrator.set_restraints`` / ``MartiniEnsembleIntegrator.set_restraints`` and
``HipMartiniSimulator(restraints=...)`` take.  Units nm, ps, kJ/mol, amu.  The laws are in include/mythos_hip.h
(mythos_martini_langevin_set_restraints); this module only describes a set and lowers it to the flat arrays of that entry
point - ``MartiniRestraints.lower`` - per replica where a value is per replica: ``init`` and ``k`` of a pull coordinate, the
references of position restraints that were left ``None``, and the box.

R umbrella windows are R replicas with their own ``init``::

    windows = np.linspace(0.0, 2.0, 8)
    rs = MartiniRestraints(pulls=[PullCoordinate(group_a=PullGroup(selection="name PO4"), group_b=PullGroup(members=[solute]),
                                                 geometry="direction", vec=(0, 0, 1), k=1000.0, init=windows)])
    sim = HipMartiniSimulator(..., temperatures=[310.0] * 8, restraints=rs)
    xi = sim.run(seed=1).state["pull"]          # (rows, 8, 1) float64 on the GPU
"""

from __future__ import annotations

import dataclasses as dc
from typing import Any, Sequence

import numpy as np

AXES = {"x": 0, "y": 1, "z": 2, 0: 0, 1: 1, 2: 2}
SHAPES = {"sphere": 0, "cylinder": 1, "layer": 2}
FLAT_PARAMS, PULL_PARAMS = 5, 9  # kMrFlatParams, kMrPullParams of csrc/martini_restraint_checks.h


@dc.dataclass(frozen=True)
class PositionRestraint:
    """U = 1/2 sum_a k_a (x_a - X_a)^2 on bead ``index``; ``k`` a scalar or per axis, >= 0; ``reference`` X (3,), or None
    for the bead's position in the ``reference_pos`` handed to ``lower`` (the loaded state)."""

    index: int
    k: Any = 1000.0
    reference: Any = None


@dc.dataclass(frozen=True)
class FlatBottomRestraint:
    """U = 1/2 k (d - r)^2 where d > r (``invert``: where d < r) on bead ``index``; ``shape`` "sphere" (d = |x - X|),
    "cylinder" (distance from the line along ``axis`` through X) or "layer" (d = |x_a - X_a|, a = ``axis``); ``reference`` X
    (3,), or None for the bead's position in ``reference_pos``."""

    index: int
    shape: str = "sphere"
    r: float = 0.0
    k: float = 1000.0
    axis: Any = "z"
    invert: bool = False
    reference: Any = None


@dc.dataclass(frozen=True)
class PullGroup:
    """The beads of one pull group: ``members`` (indices) or ``selection`` (a string or tuple for
    ``observables.membrane.select``, which needs the topology).  ``pbc_ref``: a member relative to which the others are
    taken at their minimum image (GROMACS' ``pbcatom``), for a group the input file wrapped across a face."""

    members: Any = None
    selection: Any = None
    pbc_ref: int | None = None

    def indices(self, topology=None) -> np.ndarray:
        if (self.members is None) == (self.selection is None):
            raise ValueError("PullGroup takes either members or a selection")
        if self.members is not None:
            return np.asarray(self.members, dtype=np.int64).reshape(-1)
        if topology is None:
            raise ValueError("a PullGroup given by a selection needs the topology")
        from mythos_amd.observables.membrane import select

        return np.flatnonzero(select(topology, self.selection)).astype(np.int64)


@dc.dataclass(frozen=True)
class PullCoordinate:
    """One pull coordinate between the centres of mass of ``group_a`` (None: the absolute reference point ``origin``) and
    ``group_b``.  ``kind`` "umbrella" (U = 1/2 k (xi - init - rate t)^2) or "constant-force" (U = k xi: k is the negative of
    the force, as GROMACS words it); ``geometry`` "distance" (xi = |D| over the axes of ``dim``) or "direction"
    (xi = D . vec / |vec|); ``periodic``: the minimum image of D in the replica's box.  ``init`` and ``k`` may be (R,) arrays,
    one value per replica."""

    group_b: PullGroup
    group_a: PullGroup | None = None
    kind: str = "umbrella"
    geometry: str = "distance"
    dim: Sequence[bool] = (True, True, True)
    vec: Any = (0.0, 0.0, 1.0)
    init: Any = 0.0
    rate: float = 0.0
    k: Any = 1000.0
    periodic: bool = True
    origin: Any = (0.0, 0.0, 0.0)


def _per_replica(value, n_rep: int, what: str) -> np.ndarray:
    v = np.asarray(value, dtype=np.float64)
    if v.ndim == 0:
        return np.full(n_rep, float(v))
    if v.shape != (n_rep,):
        raise ValueError(f"{what} must be a scalar or hold {n_rep} values, one per replica")
    return v.copy()


@dc.dataclass(frozen=True)
class MartiniRestraints:
    """A set: ``position`` restraints, ``flat_bottom`` restraints and ``pulls``.  Empty = no external force."""

    position: Sequence[PositionRestraint] = ()
    flat_bottom: Sequence[FlatBottomRestraint] = ()
    pulls: Sequence[PullCoordinate] = ()

    def __bool__(self) -> bool:
        return bool(len(self.position) or len(self.flat_bottom) or len(self.pulls))

    def lower(self, topology=None, n_rep: int = 1, masses=None, boxes=None, reference_pos=None) -> dict:
        """The flat arrays of mythos_martini_langevin_set_restraints for ``n_rep`` replicas: integer topology once,
        parameters per replica.  ``boxes`` (R, 3) or (3,); ``reference_pos`` (n, 3) or (R, n, 3) for the references left None.
        ``masses`` is not lowered - the library weights with the integrator's own - and is only checked for its length when a
        topology is there.  A group that several coordinates name (the same PullGroup object, or equal ones) is stored once."""
        n_rep = int(n_rep)
        if masses is not None and topology is not None and len(masses) != len(topology.atom_names):
            raise ValueError("masses must hold one value per bead of the topology")
        ref = None if reference_pos is None else np.asarray(reference_pos, dtype=np.float64)
        if ref is not None and ref.ndim == 2:
            ref = np.broadcast_to(ref, (n_rep, *ref.shape))

        def reference(index, given, what):
            if given is not None:
                return np.broadcast_to(np.asarray(given, dtype=np.float64).reshape(3), (n_rep, 3))
            if ref is None:
                raise ValueError(f"{what} of bead {index} has no reference: pass reference_pos")
            if not 0 <= int(index) < ref.shape[1]:
                raise ValueError(f"{what}: index {index} out of range [0, {ref.shape[1]})")
            return ref[:, int(index)]

        np_, nf, npl = len(self.position), len(self.flat_bottom), len(self.pulls)
        pr_index = np.array([int(p.index) for p in self.position], dtype=np.int32)
        pr_k = np.zeros((np_, 3))
        pr_ref = np.zeros((n_rep, np_, 3))
        for t, p in enumerate(self.position):
            pr_k[t] = np.broadcast_to(np.asarray(p.k, dtype=np.float64), (3,))
            pr_ref[:, t] = reference(p.index, p.reference, "position restraint")
        fb_index = np.array([int(f.index) for f in self.flat_bottom], dtype=np.int32)
        fb_flags = np.zeros(nf, dtype=np.int32)
        fb_param = np.zeros((n_rep, nf, FLAT_PARAMS))
        for t, f in enumerate(self.flat_bottom):
            if f.shape not in SHAPES or f.axis not in AXES:
                raise ValueError(f"flat-bottom restraint {t}: shape must be one of {list(SHAPES)}, axis one of x, y, z")
            fb_flags[t] = SHAPES[f.shape] | (AXES[f.axis] << 2) | (int(bool(f.invert)) << 4)
            fb_param[:, t, 0], fb_param[:, t, 1] = float(f.k), float(f.r)
            fb_param[:, t, 2:5] = reference(f.index, f.reference, "flat-bottom restraint")
        groups: list[tuple[tuple, int]] = []  # (members, pbc_ref)

        def group_id(g: PullGroup) -> int:
            key = (tuple(int(i) for i in g.indices(topology)), -1 if g.pbc_ref is None else int(g.pbc_ref))
            if key not in groups:
                groups.append(key)
            return groups.index(key)

        p_flags = np.zeros(npl, dtype=np.int32)
        p_groups = np.zeros((npl, 2), dtype=np.int32)
        p_param = np.zeros((n_rep, npl, PULL_PARAMS))
        for t, c in enumerate(self.pulls):
            if c.kind not in ("umbrella", "constant-force") or c.geometry not in ("distance", "direction"):
                raise ValueError(f"pull coordinate {t}: kind 'umbrella' or 'constant-force', geometry 'distance' or 'direction' "
                                 f"(not built: cylinder, direction-periodic)")
            dim = [bool(d) for d in c.dim]
            if len(dim) != 3:
                raise ValueError(f"pull coordinate {t}: dim holds three flags")
            p_flags[t] = (int(c.kind == "constant-force") | (int(c.geometry == "direction") << 1) | (int(bool(c.periodic)) << 2)
                          | (sum(int(d) << a for a, d in enumerate(dim)) << 4))
            p_groups[t] = (-1 if c.group_a is None else group_id(c.group_a), group_id(c.group_b))
            vec = np.asarray(c.vec, dtype=np.float64).reshape(3)
            norm = float(np.linalg.norm(vec))
            p_param[:, t, 0] = _per_replica(c.k, n_rep, f"pull coordinate {t}: k")
            p_param[:, t, 1] = _per_replica(c.init, n_rep, f"pull coordinate {t}: init")
            p_param[:, t, 2] = float(c.rate)
            p_param[:, t, 3:6] = vec / norm if norm > 0 and np.isfinite(norm) else vec  # (a zero vec is the library's to refuse)
            p_param[:, t, 6:9] = np.asarray(c.origin, dtype=np.float64).reshape(3)
        g_first = np.zeros(len(groups) + 1, dtype=np.int32)
        g_first[1:] = np.cumsum([len(m) for m, _ in groups])
        g_member = np.array([i for m, _ in groups for i in m], dtype=np.int32)
        g_pbc_ref = np.array([r for _, r in groups], dtype=np.int32)
        b = None
        if boxes is not None:
            b = np.asarray(boxes, dtype=np.float64)
            if b.shape == (3,):
                b = np.broadcast_to(b, (n_rep, 3))
            if b.shape != (n_rep, 3):
                raise ValueError(f"boxes must have shape ({n_rep}, 3), or (3,) for every replica")
        c_ = np.ascontiguousarray
        return dict(n_rep=n_rep, pr_index=c_(pr_index), pr_k=c_(pr_k), pr_ref=c_(pr_ref), fb_index=c_(fb_index), fb_flags=c_(fb_flags),
                    fb_param=c_(fb_param), g_first=c_(g_first), g_member=c_(g_member), g_pbc_ref=c_(g_pbc_ref), p_flags=c_(p_flags),
                    p_groups=c_(p_groups), p_param=c_(p_param), boxes=None if b is None else c_(b, dtype=np.float64))

    # ---- the pull subset of an .mdp ---------------------------------------------------------------------------------
    @classmethod
    def from_mdp(cls, keys: dict, groups: dict) -> "MartiniRestraints":
        """The pull coordinates of an .mdp dict (values may be the file's strings): ``pull``, ``pull-ngroups``,
        ``pull-ncoords``, ``pull-groupN-name`` / ``-pbcatom`` (1-based, 0 = none), ``pull-coordN-type`` / ``-geometry`` /
        ``-groups`` / ``-dim`` / ``-vec`` / ``-init`` / ``-rate`` / ``-k``.  ``groups``: name -> 0-based indices (``read_ndx``).
        Group 0 is GROMACS' absolute reference.  Any other key that starts with ``pull`` is refused by name."""
        import re

        mdp = {str(k).lower().replace("_", "-"): (v.strip() if isinstance(v, str) else v) for k, v in keys.items()}
        known = re.compile(r"^pull$|^pull-ngroups$|^pull-ncoords$|^pull-group\d+-(name|pbcatom)$|"
                           r"^pull-coord\d+-(type|geometry|groups|dim|vec|init|rate|k)$")
        for k in mdp:
            if k.startswith("pull") and not known.match(k):
                raise ValueError(f"from_mdp: the pull key {k!r} is not built")
        if str(mdp.get("pull", "no")).lower() not in ("yes", "true", "1"):
            return cls()
        ng, nc = int(mdp.get("pull-ngroups", 0)), int(mdp.get("pull-ncoords", 0))
        pg: dict[int, PullGroup] = {}
        for g in range(1, ng + 1):
            name = mdp.get(f"pull-group{g}-name")
            if name is None or name not in groups:
                raise ValueError(f"from_mdp: pull-group{g}-name = {name!r} is not a group of the index")
            atom = int(mdp.get(f"pull-group{g}-pbcatom", 0))
            if atom < 0:
                raise ValueError(f"from_mdp: pull-group{g}-pbcatom = {atom} is not built (an atom number, or 0)")
            pg[g] = PullGroup(members=tuple(int(i) for i in groups[name]), pbc_ref=None if atom == 0 else atom - 1)
        nums = lambda v: [float(x) for x in (v.split() if isinstance(v, str) else np.atleast_1d(v))]  # noqa: E731
        pulls = []
        for c in range(1, nc + 1):
            get = lambda key, default=None: mdp.get(f"pull-coord{c}-{key}", default)  # noqa: E731, B023
            kind, geometry = str(get("type", "umbrella")).lower(), str(get("geometry", "distance")).lower()
            if kind not in ("umbrella", "constant-force") or geometry not in ("distance", "direction"):
                raise ValueError(f"from_mdp: pull-coord{c}: type {kind!r} / geometry {geometry!r} is not built")
            ids = [int(x) for x in nums(get("groups", ""))]
            if len(ids) != 2 or not all(0 <= i <= ng for i in ids) or ids[1] == 0:
                raise ValueError(f"from_mdp: pull-coord{c}-groups must name two groups of 1 .. {ng} (the first may be 0)")
            dim = get("dim", "Y Y Y")
            dim = [str(d).upper().startswith("Y") for d in (dim.split() if isinstance(dim, str) else dim)]
            pulls.append(PullCoordinate(group_a=None if ids[0] == 0 else pg[ids[0]], group_b=pg[ids[1]], kind=kind, geometry=geometry,
                                        dim=tuple(dim), vec=tuple(nums(get("vec", "0 0 0"))), init=nums(get("init", 0.0))[0],
                                        rate=nums(get("rate", 0.0))[0], k=nums(get("k", 0.0))[0]))
        return cls(pulls=tuple(pulls))


def read_ndx(path) -> dict:
    """A GROMACS index file -> {group name: (m,) int64 array of 0-based indices} (the file counts from 1)."""
    groups: dict[str, list[int]] = {}
    name = None
    with open(path) as fh:
        for line in fh:
            line = line.split(";")[0].strip()
            if not line:
                continue
            if line.startswith("["):
                name = line.strip("[] \t")
                groups[name] = []
            elif name is None:
                raise ValueError(f"{path}: indices in front of the first [ group ]")
            else:
                groups[name].extend(int(x) - 1 for x in line.split())
    return {k: np.asarray(v, dtype=np.int64) for k, v in groups.items()}


def round_trips(window_rows) -> np.ndarray:
    """For every slot of a ``(rows, R)`` history of ``window_of_slot`` (``last_windows`` of a run with window exchange, or
    several runs' concatenated): the number of completed trips rung 0 -> rung R - 1 -> rung 0.  A trip starts counting at
    the slot's first visit to rung 0; one that has not come back by the last row does not count.  Host only; -> (R,) int64."""
    w = np.asarray(window_rows.cpu() if hasattr(window_rows, "cpu") else window_rows, dtype=np.int64)
    if w.ndim != 2:
        raise ValueError("window_rows must have shape (rows, R)")
    top = w.shape[1] - 1
    trips = np.zeros(w.shape[1], dtype=np.int64)
    if top < 1:
        return trips
    for s in range(w.shape[1]):
        state = 0  # 0: waiting for rung 0, 1: left rung 0, heading up, 2: reached the top, heading down
        for g in w[:, s]:
            if state == 0 and g == 0:
                state = 1
            elif state == 1 and g == top:
                state = 2
            elif state == 2 and g == 0:
                trips[s] += 1
                state = 1
    return trips


def check(n: int, arrays: dict, barostat: bool = False, exchange: bool = False) -> None:
    """What ``set_restraints`` refuses, without a device (mythos_martini_restraints_check), for ``arrays`` of ``lower`` and
    ``n`` beads per replica.  Raises ValueError with the library's message."""
    from mythos_amd import _lib

    _lib.check(_lib.load().mythos_martini_restraints_check(int(n), int(arrays["n_rep"]), *c_args(arrays), int(bool(barostat)),
                                                            int(bool(exchange))), "martini_restraints_check")


def c_args(a: dict) -> tuple:
    """The arguments of the two entry points behind the handle / the sizes, from the arrays of ``lower``."""
    from mythos_amd import _lib

    ip = lambda x: x.ctypes.data_as(_lib.c_int_p)  # noqa: E731
    dp = lambda x: None if x is None else x.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    return (int(a["pr_index"].shape[0]), ip(a["pr_index"]), dp(a["pr_k"]), dp(a["pr_ref"]),
            int(a["fb_index"].shape[0]), ip(a["fb_index"]), ip(a["fb_flags"]), dp(a["fb_param"]),
            int(a["g_pbc_ref"].shape[0]), ip(a["g_first"]), ip(a["g_member"]), ip(a["g_pbc_ref"]),
            int(a["p_flags"].shape[0]), ip(a["p_flags"]), ip(a["p_groups"]), dp(a["p_param"]), dp(a["boxes"]))
