"""CPU tests of the radial distribution function: the NumPy restatement (tests/rdf_ref.py) against hand-counted cases,
the host arithmetic of the observable (admissible pairs, shell volumes, normalisation) and every argument error - those of
the Python object and those of ``mythos_rdf_create``, whose host checks run in front of the device selection."""

import dataclasses as dc
import math

import numpy as np
import pytest

from mythos_amd import _lib
from mythos_amd.input.gromacs import MartiniTopology
from mythos_amd.observables import RadialDistribution, RadialDistributionPair
from mythos_amd.observables import rdf as RDF
from tests import rdf_ref as R


def _top(names, residue_index=None):
    n = len(names)
    return MartiniTopology(atom_types=("P",) * n, atom_names=tuple(names), residue_names=("MOL",) * n,
                           angles=np.zeros((0, 3), dtype=np.int32), bonded_neighbors=np.zeros((0, 2), dtype=np.int32),
                           residue_index=None if residue_index is None else np.asarray(residue_index))


# ---- the restatement against hand counts ------------------------------------------------------------------------------
def test_restatement_counts_the_neighbour_shells_of_a_simple_cubic_lattice():
    """4 x 4 x 4 cells of spacing 1 in a box of 4: every bead has 6, 12 and 8 neighbours at 1, sqrt 2 and sqrt 3, and
    nothing else below 1.9.  7 bins of 1.9 / 7: the three shells fall in bins 3, 5 and 6."""
    g = np.arange(4, dtype=np.float64)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(1, 64, 3) + 0.25  # (off the faces)
    box = np.array([[4.0, 4.0, 4.0]])
    every = np.arange(64)
    c, margin = R.counts(x, box, every, every, 7, 1.9)
    assert c.tolist() == [[0, 0, 0, 64 * 6, 0, 64 * 12, 64 * 8]]
    assert margin > 0.2
    # the lateral RDF of the same lattice: 4 beads above each other at r = 0 (3 partners each), then 4 x 4 at 1, 4 x 4 at sqrt 2
    c, _ = R.counts(x, box, every, every, 7, 1.9, dims="xy")
    assert c.tolist() == [[64 * 3, 0, 0, 64 * 16, 0, 64 * 16, 0]]
    # one layer against the next: 16 beads, each with 1 partner at 1, 4 at sqrt 2 and 4 at sqrt 3 in the layer above
    lower, upper = np.flatnonzero(x[0, :, 2] == 0.25), np.flatnonzero(x[0, :, 2] == 1.25)
    c, _ = R.counts(x, box, lower, upper, 7, 1.9)
    assert c.tolist() == [[0, 0, 0, 16, 0, 16 * 4, 16 * 4]]


def test_restatement_across_a_face_at_r_max_and_with_blocks():
    box = np.array([[4.0, 4.0, 4.0]])
    # two beads across the x face: 0.1 and 3.9 are 0.2 apart
    x = np.array([[[0.1, 1.0, 1.0], [3.9, 1.0, 1.0]]])
    c, _ = R.counts(x, box, [0], [1], 4, 1.0)
    assert c.tolist() == [[1, 0, 0, 0]]
    c, _ = R.counts(x, box, [0, 1], [0, 1], 4, 1.0)  # the same list: both orders, no self pair
    assert c.tolist() == [[2, 0, 0, 0]]
    # a pair at exactly r_max (1.5 = 1.75 - 0.25, all exact in binary) is not counted, and the margin says how close it is
    # (beads 0 - 2 are 0.3 apart, beads 1 - 2 1.53)
    x = np.array([[[0.25, 1.0, 1.0], [1.75, 1.0, 1.0], [0.25, 1.0, 1.3]]])
    c, margin = R.counts(x, box, [0, 1, 2], [0, 1, 2], 3, 1.5)
    assert c.tolist() == [[2, 0, 0]] and margin == 0.0
    c, margin = R.counts(x, box, [0, 1, 2], [0, 1, 2], 3, 1.5000001)
    assert c.tolist() == [[2, 0, 2]] and 1e-7 < margin < 1e-6
    # blocks: beads 0 and 2 share one, so only the pairs with bead 1 remain
    c, _ = R.counts(x, box, [0, 1, 2], [0, 1, 2], 4, 1.9, block=[7, 3, 7])
    assert c.sum() == 4 and R.admissible([0, 1, 2], [0, 1, 2], [7, 3, 7]).sum() == 4
    assert R.counts(x, box, [0], [1], 1, 1.6)[0].tolist() == [[1]]  # one bin


# ---- pairs, shells, normalisation ---------------------------------------------------------------------------------------
NAMES = ("A",) * 5 + ("B",) * 7 + ("C",) * 4  # 16 beads


@pytest.mark.parametrize("sel_a,sel_b", [("name A B", "name A B"), ("name A", "name B C"), ("name A B", "name B C")])
@pytest.mark.parametrize("block_size", [None, 1, 3])
def test_n_pairs_for_the_same_disjoint_and_overlapping_lists_with_and_without_blocks(sel_a, sel_b, block_size):
    resid = None if block_size is None else np.arange(16) // block_size
    top = _top(NAMES, resid if resid is not None else np.arange(16))
    obs = RadialDistribution(topology=top, pairs={"p": (sel_a, sel_b)}, r_max=1.0, n_bins=10, exclude=None if block_size is None else "residue")
    names, lists, block, n_pairs = obs.plan()
    a, b = lists[0]
    want = int(R.admissible(a, b, resid).sum())
    assert obs.n_pairs == {"p": want} and RDF.admissible_pairs(a, b, resid) == want
    by_hand = {("name A B", "name A B"): 12 * 12 - 12, ("name A", "name B C"): 5 * 11, ("name A B", "name B C"): 12 * 11 - 7}
    if block_size in (None, 1):
        assert want == by_hand[(sel_a, sel_b)]
    else:
        assert want < by_hand[(sel_a, sel_b)]
    assert (block is None) == (block_size is None)


def test_shell_volumes_and_bins():
    top = _top(NAMES)
    obs = RadialDistribution(topology=top, pairs={"p": ("name A", "name B")}, r_max=2.0, n_bins=8)
    assert np.array_equal(obs.edges, np.arange(9) * 0.25) and np.array_equal(obs.r, np.arange(8) * 0.25 + 0.125)
    v = obs.shell_volumes
    assert v.shape == (8,) and v[0] == pytest.approx(4.0 / 3.0 * math.pi * 0.25 ** 3, rel=1e-15)
    assert v[3] == pytest.approx(4.0 / 3.0 * math.pi * (1.0 - 0.75 ** 3), rel=1e-15)
    assert v.sum() == pytest.approx(4.0 / 3.0 * math.pi * 8.0, rel=1e-14)
    flat = dc.replace(obs, dims="xy")
    a = flat.shell_volumes
    assert a[3] == pytest.approx(math.pi * (1.0 - 0.75 ** 2), rel=1e-15) and a.sum() == pytest.approx(math.pi * 4.0, rel=1e-14)
    assert np.allclose(R.shells(8, 2.0), v, rtol=1e-15) and np.allclose(R.shells(8, 2.0, "xy"), a, rtol=1e-15)
    with pytest.raises(ValueError, match="expected 'xyz' or 'xy'"):
        RDF.shell_volumes(obs.edges, "xz")


def test_normalisation_of_the_restatement_gives_one_for_an_ideal_count():
    """counts = N_pairs v_b / V_f exactly -> g = 1, with a box of its own per frame; and in xy."""
    box = np.array([[4.0, 5.0, 6.0], [4.5, 5.0, 7.0]])
    for dims, vol in (("xyz", box.prod(1)), ("xy", box[:, 0] * box[:, 1])):
        ideal = 1000.0 * R.shells(5, 1.5, dims)[None, :] / vol[:, None]
        g = ideal * vol[:, None] / (1000.0 * R.shells(5, 1.5, dims))[None, :]
        assert np.allclose(g, 1.0, rtol=1e-15)
    c = np.array([[3, 0, 7], [1, 2, 0]])
    g = R.g_of(c, box, 11, 1.5)
    assert g[0, 2] == pytest.approx(7 * 120.0 / (11 * 4.0 / 3.0 * math.pi * (1.5 ** 3 - 1.0)), rel=1e-14)
    assert g[1, 1] == pytest.approx(2 * 157.5 / (11 * 4.0 / 3.0 * math.pi * (1.0 - 0.125)), rel=1e-14) and g[0, 1] == 0.0


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_selection_and_argument_errors():
    top = _top(NAMES, np.arange(16) // 4)
    ok = dict(topology=top, pairs={"p": ("name A", "name B")}, r_max=1.0, n_bins=10)
    RadialDistribution(**ok)
    with pytest.raises(ValueError, match="selection 'name W' matches no bead of the topology"):
        RadialDistribution(**{**ok, "pairs": {"p": ("name A", "name W")}})
    with pytest.raises(ValueError, match="unsupported token"):
        RadialDistribution(**{**ok, "pairs": {"p": ("name A", "around 5 name B")}})
    with pytest.raises(ValueError, match=r"pair 'p': expected \(selection A, selection B\)"):
        RadialDistribution(**{**ok, "pairs": {"p": "name A"}})
    with pytest.raises(ValueError, match="pairs: expected at least one"):
        RadialDistribution(**{**ok, "pairs": {}})
    for bad in (0, 4097, 2.5):
        with pytest.raises(ValueError, match="n_bins"):
            RadialDistribution(**{**ok, "n_bins": bad})
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="r_max"):
            RadialDistribution(**{**ok, "r_max": bad})
    with pytest.raises(ValueError, match="dims 'xz': expected 'xyz' or 'xy'"):
        RadialDistribution(**{**ok, "dims": "xz"})
    with pytest.raises(ValueError, match="exclude 'molecule': expected 'residue' or None"):
        RadialDistribution(**{**ok, "exclude": "molecule"})
    with pytest.raises(ValueError, match="needs topology.residue_index"):
        RadialDistribution(**{**ok, "topology": _top(NAMES), "exclude": "residue"})
    # no admissible pair: one bead against itself; two selections inside one residue
    one = _top(("A", "B", "C", "C"), [0, 0, 1, 1])
    with pytest.raises(ValueError, match="pair 'self': no admissible pair of beads .* is the same bead"):
        RadialDistribution(topology=one, pairs={"self": ("name A", "name A")}, r_max=1.0, n_bins=4)
    with pytest.raises(ValueError, match="pair 'intra': no admissible pair of beads .* shares a residue"):
        RadialDistribution(topology=one, pairs={"intra": ("name A", "name B")}, r_max=1.0, n_bins=4, exclude="residue")
    # the single-pair form checks the same
    with pytest.raises(ValueError, match="matches no bead"):
        RadialDistributionPair(topology=top, sel_a="name A", sel_b="name W", r_max=1.0, n_bins=10)
    assert RadialDistributionPair(topology=top, sel_a="name A", sel_b=("B", "C"), r_max=1.0, n_bins=10).n_pairs == {"pair": 55}

    @dc.dataclass
    class NoBox:
        center: object

    with pytest.raises(ValueError, match="need trajectory.box_size"):
        RadialDistribution(**ok)(NoBox(center=np.zeros((1, 16, 3))))


def _create(n=6, n_a=(2,), n_b=(2,), index=(0, 1, 2, 3), block=None, n_bins=8, r_max=1.0, dims=3):
    lib = _lib.load()
    arr = [np.ascontiguousarray(v, dtype=np.int32) for v in (n_a, n_b, index)]
    blk = None if block is None else np.ascontiguousarray(block, dtype=np.int32)
    h = lib.mythos_rdf_create(n, len(n_a), *(a.ctypes.data_as(_lib.c_int_p) for a in arr),
                              None if blk is None else blk.ctypes.data_as(_lib.c_int_p), n_bins, r_max, dims, 0)
    return h, _lib.last_error()


@pytest.mark.parametrize("kwargs,message", [
    (dict(index=(0, 1, 2, 6)), "bead index out of range"),
    (dict(index=(-1, 1, 2, 3)), "bead index out of range"),
    (dict(n_a=(0,), index=(2, 3)), "every list holds at least one bead"),
    (dict(n_b=(0,), index=(0, 1)), "every list holds at least one bead"),
    (dict(n_bins=0), "n_bins must be in [1, 4096]"),
    (dict(n_bins=4097), "n_bins must be in [1, 4096]"),
    (dict(r_max=0.0), "r_max must be positive and finite"),
    (dict(r_max=float("nan")), "r_max must be positive and finite"),
    (dict(dims=1), "dims must be MYTHOS_RDF_XY or MYTHOS_RDF_XYZ"),
    (dict(n_a=(), n_b=(), index=(0,)), "at least one group"),
    (dict(n_a=(1,), n_b=(1,), index=(4, 4)), "a group has no admissible pair"),
    (dict(block=(0, 0, 0, 0, 1, 1)), "a group has no admissible pair"),
    (dict(n_a=(2, 1), n_b=(2, 1), index=(0, 1, 4, 5, 3, 3)), "a group has no admissible pair"),
])
def test_create_refuses_bad_arguments_in_front_of_the_device(kwargs, message):
    h, msg = _create(**kwargs)
    assert not h and msg == f"mythos_rdf_create: {message}"
