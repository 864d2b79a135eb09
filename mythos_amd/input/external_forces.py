"""oxDNA external-force files (the ``external_forces_file`` of an oxDNA input; the reference ships eight of them under
data/templates/force-ext/externals/): the constant forces ``LangevinIntegrator.set_external_forces`` and
``HipMDSimulator(external_forces=...)`` take.

A file is a sequence of blocks ::

    {
    type = string
    particle = 5,214
    F0 = 0.025
    rate = 0.
    dir = 0., 0., 1.
    }

``type = string`` with ``rate = 0`` is a constant force ``F0 * dir / |dir|`` (oxDNA normalises ``dir``) on the centre of
mass of EACH listed particle; ``particle`` is one index, a comma-separated list (``a-b`` ranges included), or ``-1`` for
every particle.  ``read_external_forces`` reads nothing else: any other ``type`` (traps, twist, ...) and a moving force
(``rate != 0``) raise a ``ValueError`` that names the offender.  ``read_external_field`` reads the point forces as well -
moving strings, ``trap``, ``mutual_trap``, ``repulsion_plane``, ``repulsion_sphere`` - and refuses ``twist``, ``com`` and
the rest by name.  Indices are oxDNA's particle indices, the order of the topology file.
"""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np

_BLOCK = re.compile(r"\{([^{}]*)\}", re.S)


def _particles(text: str, n, where: str) -> list[int]:
    out: list[int] = []
    for tok in (t.strip() for t in text.split(",")):
        if not tok:
            continue
        m = re.fullmatch(r"(\d+)\s*-\s*(\d+)", tok)
        if m:
            out.extend(range(int(m.group(1)), int(m.group(2)) + 1))
        elif int(tok) == -1:
            if n is None:
                raise ValueError(f"{where}: particle = -1 (every particle) needs the number of nucleotides, n")
            out.extend(range(int(n)))
        else:
            out.append(int(tok))
    if not out:
        raise ValueError(f"{where}: no particle listed")
    for i in out:
        if i < 0 or (n is not None and i >= n):
            raise ValueError(f"{where}: particle {i} out of range" + ("" if n is None else f" [0, {n})"))
    return out


def sum_repeated(index, force) -> tuple[np.ndarray, np.ndarray]:
    """Forces of repeated indices summed: -> (sorted distinct int32 (m,), float64 (m, 3))."""
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    force = np.asarray(force, dtype=np.float64).reshape(-1, 3)
    if index.shape[0] != force.shape[0]:
        raise ValueError(f"{index.shape[0]} indices for {force.shape[0]} force vectors")
    uniq, inv = np.unique(index, return_inverse=True)
    total = np.zeros((uniq.shape[0], 3), dtype=np.float64)
    np.add.at(total, inv, force)
    return uniq.astype(np.int32), total


def _blocks(path):
    """The blocks of a file, comments removed: (where, {key: value}) per block, in the file's order."""
    text = "\n".join(line.split("#", 1)[0] for line in Path(path).read_text().splitlines())
    for k, body in enumerate(_BLOCK.findall(text)):
        kv = {}
        for line in body.splitlines():
            if "=" in line:
                key, val = line.split("=", 1)
                kv[key.strip()] = val.strip()
        yield f"{path}: block {k}", kv


def _need(kv, where, *keys) -> None:
    for need in keys:
        if need not in kv:
            raise ValueError(f"{where}: missing {need}")


def _vector(kv, key, where) -> np.ndarray:
    v = np.array([float(x) for x in kv[key].split(",")], dtype=np.float64)
    if v.shape != (3,):
        raise ValueError(f"{where}: {key} = {kv[key]} is not three numbers")
    return v


def _direction(kv, where) -> np.ndarray:
    """``dir`` as written, checked to be a direction (oxDNA normalises it: the callers divide by its length)."""
    d = np.array([float(x) for x in kv["dir"].split(",")], dtype=np.float64)
    if d.shape != (3,) or not np.linalg.norm(d) > 0:
        raise ValueError(f"{where}: dir = {kv['dir']} is not a direction")
    return d


def read_external_forces(path, n: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """-> (index int32 (m,), force float64 (m, 3)), one row per forced particle, a particle named more than once summed."""
    index: list[int] = []
    force: list[np.ndarray] = []
    for where, kv in _blocks(path):
        kind = kv.get("type")
        if kind != "string":
            raise ValueError(f"{where}: external force of type = {kind} is not supported (only type = string, a constant force)")
        rate = float(kv.get("rate", "0"))
        if rate != 0.0:
            raise ValueError(f"{where}: rate = {kv['rate']} (a moving force) is not supported, only rate = 0")
        _need(kv, where, "particle", "F0", "dir")
        d = _direction(kv, where)
        f = float(kv["F0"]) * d / np.linalg.norm(d)
        for i in _particles(kv["particle"], n, where):
            index.append(i)
            force.append(f)
    if not index:
        return np.zeros(0, dtype=np.int32), np.zeros((0, 3), dtype=np.float64)
    return sum_repeated(index, np.array(force))


def read_external_field(path, n: int | None = None):
    """The whole external field of a file -> (PointForces, (index, force)): the point forces
    ``LangevinIntegrator.set_point_forces`` and ``HipMDSimulator(point_forces=...)`` take, in the file's order, and the
    constant strings (``rate = 0``) as the pair ``set_external_forces`` takes.  Read: ``string``, ``trap``, ``mutual_trap``
    (``rate`` and ``PBC`` default to 0), ``repulsion_plane``, ``repulsion_sphere`` (``rate`` defaults to 0), each by oxDNA's
    definition, on every listed particle.  ``twist`` (a body torque), ``com`` and anything else raise a ``ValueError``
    that names the type."""
    from mythos_amd.simulators.restraints import MovingString, MutualTrap, PointForces, RepulsionPlane, RepulsionSphere, Trap

    terms: list = []
    index: list[int] = []
    force: list[np.ndarray] = []
    for where, kv in _blocks(path):
        kind = kv.get("type")
        if kind not in ("string", "trap", "mutual_trap", "repulsion_plane", "repulsion_sphere"):
            raise ValueError(f"{where}: external force of type = {kind} is not supported (string, trap, mutual_trap, "
                             "repulsion_plane and repulsion_sphere are)")
        _need(kv, where, "particle")
        rate = float(kv.get("rate", "0"))
        particles = _particles(kv["particle"], n, where)
        if kind == "string":
            _need(kv, where, "F0", "dir")
            d = _direction(kv, where)
            if rate == 0.0:
                index.extend(particles)
                force.extend([float(kv["F0"]) * d / np.linalg.norm(d)] * len(particles))
            else:
                terms.extend(MovingString(i, float(kv["F0"]), rate, d) for i in particles)
        elif kind == "trap":
            _need(kv, where, "pos0", "stiff", "dir")
            d, pos0 = _direction(kv, where), _vector(kv, "pos0", where)
            terms.extend(Trap(i, pos0, float(kv["stiff"]), rate, d) for i in particles)
        elif kind == "mutual_trap":
            _need(kv, where, "ref_particle", "stiff", "r0")
            (ref,) = _particles(kv["ref_particle"], n, where + " (ref_particle)")[:1]
            pbc = bool(int(kv.get("PBC", "0")))
            terms.extend(MutualTrap(i, ref, float(kv["stiff"]), float(kv["r0"]), rate, pbc) for i in particles)
        elif kind == "repulsion_plane":
            _need(kv, where, "stiff", "dir", "position")
            d = _direction(kv, where)
            terms.extend(RepulsionPlane(i, float(kv["stiff"]), d, float(kv["position"])) for i in particles)
        else:
            _need(kv, where, "center", "r0", "stiff")
            c = _vector(kv, "center", where)
            terms.extend(RepulsionSphere(i, c, float(kv["r0"]), float(kv["stiff"]), rate) for i in particles)
    const = sum_repeated(index, np.array(force)) if index else (np.zeros(0, dtype=np.int32), np.zeros((0, 3), dtype=np.float64))
    return PointForces(terms), const
