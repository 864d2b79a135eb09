"""The restraints of a LAMMPS input, as far as the reference's stretch-torsion protocol uses them
(data/templates/lammps-stretch-tors/in, tests/golden/regr/lammps-oxdna2-40bp/in): what
``HipMDSimulator(restraints=..., external_forces=...)`` takes.

Read ::

    group NAME id <= a | id >= a | id < a | id > a | id <> a b | id a b ...
    group NAME union NAME1 NAME2 ...
    variable X equal -K*(c_xu[a]+c_xu[b])         (c_yu, c_zu alike)
    fix ID GROUP spring/self K xyz                 -> SelfTether of every atom of the group to its initial position
    fix ID GROUP addtorque Tx Ty Tz                -> GroupTorque
    fix ID GROUP addforce v_X v_Y fz               -> SumRestraint(k = K, axes of the variable components, target 0: the
                                                      variable restrains the sum of the coordinates to the origin, where
                                                      the protocol's ``displace_atoms`` has put it) + the constant force
                                                      (0, 0, fz) on every atom of the group
    fix ID GROUP addforce fx fy fz                 -> a constant force on every atom of the group

Atom ids are 1-based, the indices returned 0-based; an open-ended group (``id >= a``) needs the number of atoms, ``n``
(the data file is not read).  Any other form of ``fix ... addforce``,
``addtorque`` or ``spring*`` raises a ValueError that names the line; other fixes (the integrator) are none of this
module's business and are skipped.
"""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np

from mythos_amd.input.external_forces import sum_repeated
from mythos_amd.simulators.restraints import GroupTorque, Restraints, SelfTether, SumRestraint

_NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"
_SUM_VAR = re.compile(rf"^-\s*({_NUM})\s*\*\s*\(\s*c_([xyz])u\[(\d+)\]((?:\s*\+\s*c_[xyz]u\[\d+\])*)\s*\)$")
_MORE = re.compile(r"c_([xyz])u\[(\d+)\]")


def _is_number(tok: str) -> bool:
    return re.fullmatch(_NUM, tok) is not None


def _group_ids(args: list[str], groups: dict, n, where: str) -> list[int]:
    style = args[0]
    if style == "union":
        ids: list[int] = []
        for name in args[1:]:
            if name not in groups:
                raise ValueError(f"{where}: group {name} is not defined")
            ids.extend(i for i in groups[name] if i not in ids)
        return sorted(ids)
    if style != "id":
        raise ValueError(f"{where}: group style {style} is not supported (id, union)")
    rest = args[1:]

    def ids_of(toks):
        if not all(re.fullmatch(r"\d+", v) for v in toks):
            raise ValueError(f"{where}: group ids must be plain positive integers (ranges such as 1:4 are not supported)")
        return [int(v) for v in toks]

    if rest and rest[0] in ("<=", ">=", "<", ">", "<>"):
        op, vals = rest[0], ids_of(rest[1:])
        if len(vals) != (2 if op == "<>" else 1):
            raise ValueError(f"{where}: group id {op} takes {'two ids' if op == '<>' else 'one id'}")
        if op == "<>":
            return list(range(vals[0], vals[1] + 1))
        if op in ("<=", "<"):
            return list(range(1, vals[0] + (1 if op == "<=" else 0)))
        if n is None:
            raise ValueError(f"{where}: an open-ended group (id {op} {vals[0]}) needs the number of atoms, n")
        return list(range(vals[0] + (0 if op == ">=" else 1), int(n) + 1))
    return ids_of(rest)


def read_lammps_restraints(path, n: int | None = None):
    """-> (Restraints, (index int32 (m,), force float64 (m, 3))): the position-dependent fixes, and the constant forces
    summed per atom.  ``n``: the number of atoms, for groups such as ``id >= 79``."""
    groups: dict[str, list[int]] = {}
    variables: dict[str, str] = {}
    tethers, sums, torques = [], [], []
    c_index: list[int] = []
    c_force: list[list[float]] = []
    for ln, raw in enumerate(Path(path).read_text().splitlines(), 1):
        line = raw.split("#", 1)[0].strip()
        tok = line.split()
        if not tok:
            continue
        where = f"{path}:{ln}: {line!r}"
        if tok[0] == "group" and len(tok) >= 3:
            if tok[2] in ("id", "union"):
                groups[tok[1]] = _group_ids(tok[2:], groups, n, where)
            continue  # (other group styles - type, molecule - define groups no restraint here may use: caught below)
        if tok[0] == "variable" and len(tok) >= 4 and tok[2] == "equal":
            variables[tok[1]] = "".join(tok[3:])
            continue
        if tok[0] != "fix" or len(tok) < 4:
            continue
        style, args = tok[3], tok[4:]
        if not (style in ("addforce", "addtorque") or style.startswith("spring")):
            continue
        if tok[2] not in groups:
            raise ValueError(f"{where}: group {tok[2]} is not an id / union group this reader builds")
        index = [i - 1 for i in groups[tok[2]]]
        if style == "spring/self" and len(args) in (1, 2) and _is_number(args[0]):
            axes_txt = args[1] if len(args) == 2 else "xyz"
            if not re.fullmatch(r"[xyz]{1,3}", axes_txt):
                raise ValueError(f"{where}: unsupported spring/self direction {axes_txt}")
            tethers.append(SelfTether(index, float(args[0]), None, tuple(int(a in axes_txt) for a in "xyz")))
        elif style == "addtorque" and len(args) == 3 and all(_is_number(a) for a in args):
            torques.append(GroupTorque(index, tuple(float(a) for a in args)))
        elif style == "addforce" and len(args) == 3:
            const = [0.0, 0.0, 0.0]
            axes, k_sum, members = [0, 0, 0], None, None
            for a, arg in enumerate(args):
                if _is_number(arg):
                    const[a] = float(arg)
                    continue
                m = _SUM_VAR.match(variables.get(arg[2:], "")) if arg.startswith("v_") else None
                if m is None:
                    raise ValueError(f"{where}: addforce component {arg} is not a number or a variable of the form -K*(c_xu[a]+c_xu[b])")
                comps = [(m.group(2), int(m.group(3)))] + [(c, int(i)) for c, i in _MORE.findall(m.group(4))]
                if any(c != "xyz"[a] for c, _ in comps):
                    raise ValueError(f"{where}: variable {arg[2:]} on component {'xyz'[a]} reads other coordinates")
                ids = sorted(i for _, i in comps)
                if ids != sorted(groups[tok[2]]):
                    raise ValueError(f"{where}: variable {arg[2:]} sums atoms {ids}, the fix acts on {sorted(groups[tok[2]])}")
                if (k_sum is not None and float(m.group(1)) != k_sum) or (members is not None and ids != members):
                    raise ValueError(f"{where}: the variable components differ in stiffness or atoms")
                k_sum, members, axes[a] = float(m.group(1)), ids, 1
            if k_sum is not None:
                sums.append(SumRestraint(index, k_sum, (0.0, 0.0, 0.0), tuple(axes)))
            if any(const):
                c_index.extend(index)
                c_force.extend([const] * len(index))
        else:
            raise ValueError(f"{where}: fix {style} in this form is not supported "
                             "(spring/self K [xyz], addtorque Tx Ty Tz, addforce with numbers or sum variables)")
    forces = sum_repeated(c_index, np.array(c_force).reshape(-1, 3)) if c_index else (np.zeros(0, np.int32), np.zeros((0, 3)))
    return Restraints(tethers=tethers, sums=sums, torques=torques), forces
