"""Synthetic oxDNA systems for benchmarks and tests (the reference ships nothing above 1000 nt).

``ideal_duplex`` builds a straight B-form double helix in oxDNA rigid-body coordinates:
centre of mass 0.6 length units from the helix axis with a1 pointing at the axis, rise
0.3897628551303122 units per base pair, 10.5 bp per turn (oxDNA2; 10.34 for oxDNA1), right-handed;
strand 2 is antiparallel with a1, a3 reversed.  Memory order is oxDNA-classic 3'->5' per strand,
strand 1 first, so bonded pairs are (k, k+1) exactly as mythos/input/topology.py:166-183 produces.
"""

from __future__ import annotations

import numpy as np

from mythos_amd.input import topology as jd_top
from mythos_amd.input.trajectory import axes_to_quaternion

BASE_BASE = 0.3897628551303122
CM_CENTER_DS = 0.6


def _rot(axis: np.ndarray, angle: float) -> np.ndarray:
    axis = axis / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def ideal_duplex(n_bp: int, *, model: int = 2, seed: int = 1234, origin=(0.0, 0.0, 0.0), axis=(0.0, 0.0, 1.0), seq=None):
    """Returns (topology, center (2n,3), quaternion (2n,4)) in float64."""
    rng = np.random.default_rng(seed)
    seq1 = rng.integers(0, 4, n_bp) if seq is None else np.asarray(seq, dtype=np.int64)
    if seq1.shape != (n_bp,):
        raise ValueError("seq must have one entry per base pair")
    bp_per_turn = 10.5 if model == 2 else 10.34
    step = 2.0 * np.pi / bp_per_turn
    d = np.asarray(axis, dtype=np.float64)
    d = d / np.linalg.norm(d)
    # any unit vector perpendicular to the axis
    trial = np.array([1.0, 0.0, 0.0]) if abs(d[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    a1 = np.cross(d, trial)
    a1 /= np.linalg.norm(a1)
    R = _rot(d, step)
    rb = np.asarray(origin, dtype=np.float64).copy()
    c1, a11, a31 = [], [], []
    for _ in range(n_bp):
        c1.append(rb - CM_CENTER_DS * a1)
        a11.append(a1.copy())
        a31.append(d.copy())
        a1 = R @ a1
        rb = rb + d * BASE_BASE
    c1, a11, a31 = np.array(c1), np.array(a11), np.array(a31)
    # strand 2: nucleotide j pairs with nucleotide n-1-j of strand 1
    c2 = (c1 + 2 * CM_CENTER_DS * a11)[::-1]
    a12 = (-a11)[::-1]
    a32 = (-a31)[::-1]
    seq2 = (3 - seq1)[::-1]
    center = np.concatenate([c1, c2])
    a1s = np.concatenate([a11, a12])
    a3s = np.concatenate([a31, a32])
    quat = axes_to_quaternion(a1s, a3s)
    top = jd_top.from_arrays(np.concatenate([seq1, seq2]).astype(np.int32), [n_bp, n_bp])
    return top, np.ascontiguousarray(center), np.ascontiguousarray(quat)


def tiled_martini_box(topology, positions, box, reps: int):
    """A MARTINI box repeated ``reps`` x ``reps`` times in-plane (x, y) -> (tiled topology, positions, box).
    GROMACS wraps bead by bead, so every molecule is made whole first (each bead's first bond partner has a lower
    index); otherwise a bond that crossed a face would span a whole tile."""
    x0, b0 = np.array(positions, dtype=np.float64), np.asarray(box, dtype=np.float64)
    for i, j in topology.bonded_neighbors:
        d = x0[j] - x0[i]
        x0[j] = x0[i] + d - b0 * np.round(d / b0)
    xt = np.concatenate([x0 + np.array([i * b0[0], j * b0[1], 0.0]) for i in range(reps) for j in range(reps)])
    return topology.tile(reps * reps), xt, b0 * np.array([reps, reps, 1.0])


def duplex_bundle(n_bp: int, n_duplexes: int, spacing: float = 6.0, **kw):
    """Several parallel duplexes on a square lattice (independent molecules in one system)."""
    side = int(np.ceil(np.sqrt(n_duplexes)))
    seqs, counts, cs, qs = [], [], [], []
    for k in range(n_duplexes):
        top, c, q = ideal_duplex(n_bp, seed=kw.get("seed", 1234) + k, origin=(spacing * (k % side), spacing * (k // side), 0.0), model=kw.get("model", 2))
        seqs.append(top.seq)
        counts += [n_bp, n_bp]
        cs.append(c)
        qs.append(q)
    top = jd_top.from_arrays(np.concatenate(seqs), counts)
    return top, np.concatenate(cs), np.concatenate(qs)
