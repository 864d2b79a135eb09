"""Deterministic oxDNA configurations in periodic boxes whose faces the strands cross (NumPy only), for the MD tests:
the golden helices sit in the middle of their 20-unit box, and every MD test with a device-built list runs in free space.

Every generator returns ``(topology, centre, quaternion, box)`` in float64; ``box`` is a (3,) array.

``crossing_helix(model, name)``: frame 0 of a golden system, translated rigidly so that its centroid lies next to the
corner (L, 0, L) of the box - the molecule then straddles a face of each axis, with mixed signs of the image along
them -, after which its second strand is moved by the lattice vector (-L, +L, -L): every H-bond, cross-stack and
excluded-volume pair between the strands goes through an image in all three components.  ``name == "circular"`` is
the system of tests/test_gpu_edge_cases.py (dna2/simple-helix with a circular first strand): there the second half of
the ring is moved by (+L, -L, +L) as well, so two bonded pairs - FENE, stacking - go through an image too.  The
translation is a multiple of 2^-6, so a configuration that is representable in fp32 stays so.  ``placement`` returns
the whole golden frame and the displacement of every nucleotide separately.

``duplex_lattice(box_x)``: 24 perturbed ideal 12-bp duplexes (576 nt, the cell builder's threshold is 512) along z on a
2 x 6 x 2 grid that is periodic with the box (box_x, 39, 13), translated by (box_x - 0.25, 38.75, 11.5): the coordinates
are unwrapped and cross every face, and a duplex - centres 0.6 from its axis - lies across a face of each axis, so listed
pairs straddle all of them (a translation of (box_x - 1, 37, .) would leave the nearest axes 1 and 2 units from the x and
y faces: no pair would).  At a list range of 3.85 (cut-off 3.25 + skin 0.6) box_x = 13 gives 3 x 10 x 3 cells -
the 27-cell stencil covers x and z exactly once -, box_x = 11 only two cells along x, where the all-pairs builder takes
over and the minimum image alone decides.

``wrapped(c, box)``: the same configuration with every centre folded into [0, L), nucleotide by nucleotide.
"""

from __future__ import annotations

import functools

import numpy as np

from mythos_amd.input import topology
from mythos_amd.utils import generators
from tests import helpers as H

CROSSING = ((1, "simple-helix"), (2, "simple-helix"), (3, "simple-helix-12bp"), (4, "simple-helix-dna-rna"), (2, "circular"))
SALT = {1: 0.5, 2: 0.5, 3: 1.0, 4: 0.5}
STRAND_IMAGE = np.array([-1.0, 1.0, -1.0])  # lattice vector of the second strand, in box edges
RING_IMAGE = np.array([1.0, -1.0, 1.0])     # ... of the second half of a circular first strand
GRID = 64.0

R_CUT, SKIN = 3.25, 0.6
LATTICE_BOX_YZ = (39.0, 13.0)
LATTICE_N = 576


def golden_frame(model: int, name: str):
    """(topology, centre, quaternion, box (3,)) of frame 0 of a golden system, as stored."""
    if model == 4:
        top, traj, _, _ = H.load_golden_na1(name)
    elif name == "circular":
        ref_top, traj, _, _ = H.load_golden(2, "simple-helix")
        top = topology.from_arrays(ref_top.seq, ref_top.strand_counts, is_circular=[True, False])
    else:
        top, traj, _, _ = H.load_golden(model, name)
    box = np.broadcast_to(np.asarray(traj.box_size, dtype=np.float64), (3,)).copy()
    return top, np.array(traj.center[0], dtype=np.float64), np.array(traj.quaternions[0], dtype=np.float64), box


@functools.lru_cache(maxsize=None)
def _placement(model: int, name: str):
    top, c, q, box = golden_frame(model, name)
    corner = box * np.array([1.0, 0.0, 1.0])
    shift = np.round((corner - c.mean(0)) * GRID) / GRID
    move = np.tile(shift, (c.shape[0], 1))
    n0 = int(top.strand_counts[0])
    move[n0:] += STRAND_IMAGE * box
    if name == "circular":
        move[n0 // 2:n0] += RING_IMAGE * box
    return top, c, q, box, move


def placement(model: int, name: str):
    """(topology, the whole golden frame's centres, quaternions, box, displacement (N, 3) that makes it cross)."""
    top, c, q, box, move = _placement(model, name)
    return top, c.copy(), q.copy(), box.copy(), move.copy()


def crossing_helix(model: int, name: str):
    top, c, q, box, move = placement(model, name)
    return top, c + move, q, box


def is_rna(top):
    return np.asarray(top.nt_type) == int(topology.NucleotideType.RNA)


@functools.lru_cache(maxsize=None)
def _lattice(box_x: float):
    seqs, counts, cs, qs = [], [], [], []
    k = 0
    for ix in range(2):
        for iy in range(6):
            for iz in range(2):
                top, c, q = generators.ideal_duplex(12, model=2, seed=100 + k, origin=(0.5 * box_x * ix, 6.5 * iy, 6.5 * iz))
                seqs.append(top.seq)
                counts += [12, 12]
                cs.append(c)
                qs.append(q)
                k += 1
    top = topology.from_arrays(np.concatenate(seqs).astype(np.int32), counts)
    c, q = np.concatenate(cs), np.concatenate(qs)
    rng = np.random.default_rng(int(round(box_x)))
    c = c + 0.015 * rng.standard_normal(c.shape)
    q = q + 0.0075 * rng.standard_normal(q.shape)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    c = c + np.array([box_x - 0.25, 38.75, 11.5])
    return top, np.ascontiguousarray(c), np.ascontiguousarray(q), np.array([box_x, *LATTICE_BOX_YZ])


def duplex_lattice(box_x: float):
    top, c, q, box = _lattice(float(box_x))
    return top, c.copy(), q.copy(), box.copy()


def wrapped(c, box):
    return np.mod(c, np.asarray(box, dtype=np.float64))


def cells_per_edge(box, r_list=R_CUT + SKIN):
    """What cell_grid (mythos_amd/csrc/cell_list.h) makes of a box: floor(L / list range) cells per edge; under three
    on any edge the all-pairs builder takes over."""
    return tuple(int(np.floor(edge / r_list)) for edge in np.asarray(box, dtype=np.float64))


def image_of_pairs(c, pairs, box):
    """(P, 3) integers: the lattice vector, in box edges, that the minimum image subtracts from c[j] - c[i]."""
    d = c[pairs[:, 1]] - c[pairs[:, 0]]
    return np.rint(d / np.asarray(box, dtype=np.float64)).astype(np.int64)
