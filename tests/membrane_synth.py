"""Deterministic synthetic bilayers for the membrane tests (NumPy only): lipid counts, residue mixes and frames that
the 128-lipid golden membrane never reaches.

A system is a list of residues, each of a kind and a side:
  "ten"  a ten-bead lipid (NC3 PO4 GL1 GL2 C1A C2A C3A C1B C2B C3B, residue LIP): two beads of the lipid selection
         ``name GL1 GL2`` and one of the thickness selection ``name PO4``
  "one"  a one-bead lipid (GL1, residue ONE): one bead of the lipid selection, no thickness bead
  "w"    a three-bead residue W that owns no selected bead, anywhere in z
side +1 / -1 puts a lipid's selected beads 0.6 - 1.2 nm above / below the plane z = LZ / 2, re-drawn in every frame; the
midpoint of the selection's beads stays within 0.3 nm of that plane for the mixes used here, and ``get`` asserts with
the restatement (tests/membrane_ref.py) that no lipid is within 1e-6 nm of the midpoint - leaflets then compare as
integers.  The two deliberate exact ties ("tie", and "empty_upper", where an empty upper leaflet REQUIRES every lipid
to sit exactly at the midpoint, a weighted mean of the lipids) are built from exactly representable numbers.
"""

from __future__ import annotations

import functools

import numpy as np

from mythos_amd.input.gromacs import MartiniTopology
from tests import membrane_ref as R

LZ = 10.0
TEN = ("NC3", "PO4", "GL1", "GL2", "C1A", "C2A", "C3A", "C1B", "C2B", "C3B")
TEN_OFFSET = np.array([1.0, 0.6, 0.0, 0.0, -0.2, -0.35, -0.5, -0.2, -0.35, -0.5])  # outwards from the selected beads
LIPID_SEL, THICKNESS_SEL = "name GL1 GL2", "name PO4"


def topology(kinds) -> MartiniTopology:
    names, res, resid = [], [], []
    for r, kind in enumerate(kinds):
        beads, resname = {"ten": (TEN, "LIP"), "one": (("GL1",), "ONE"), "w": (("W",) * 3, "W")}[kind]
        names += beads
        res += [resname] * len(beads)
        resid += [r] * len(beads)
    n = len(names)
    return MartiniTopology(atom_types=("P",) * n, atom_names=tuple(names), residue_names=tuple(res),
                           angles=np.zeros((0, 3), dtype=np.int32), bonded_neighbors=np.zeros((0, 2), dtype=np.int32),
                           residue_index=np.array(resid, dtype=np.int32))


def make(kinds, sides, frames, seed, vary_box=False, flips=()) -> dict:
    """``sides`` per residue (ignored for "w"); ``flips``: (residue, frame) pairs whose lipid sits on the other side in
    that frame."""
    rng = np.random.default_rng(seed)
    top = topology(kinds)
    n = len(top.atom_names)
    box = np.tile([6.0, 7.0, LZ], (frames, 1))
    if vary_box:
        box[:, 0] += 0.01 * np.arange(frames)
        box[:, 1] -= 0.013 * np.arange(frames)
    x = np.zeros((frames, n, 3))
    flips = set(flips)
    for f in range(frames):
        at = 0
        for r, (kind, side) in enumerate(zip(kinds, sides)):
            if (r, f) in flips:
                side = -side
            if kind == "ten":
                z = 0.5 * LZ + side * (rng.uniform(0.6, 1.2) + TEN_OFFSET + rng.uniform(-0.05, 0.05, size=10))
            elif kind == "one":
                z = 0.5 * LZ + side * rng.uniform(0.6, 1.2, size=1)
            else:
                z = rng.uniform(0.0, LZ, size=3)
            m = len(z)
            x[f, at:at + m, 0] = rng.uniform(0.0, box[f, 0], size=m)
            x[f, at:at + m, 1] = rng.uniform(0.0, box[f, 1], size=m)
            x[f, at:at + m, 2] = z
            at += m
    return dict(top=top, x=x, box=box, lipid_sel=LIPID_SEL, thickness_sel=THICKNESS_SEL, exact_tie=False)


def _exact(zs, frames=1) -> dict:
    """Ten-bead lipids with every bead of a lipid at that lipid's z (small integers: every sum and mean is exact)."""
    kinds = ["ten"] * len(zs)
    top = topology(kinds)
    x = np.zeros((frames, 10 * len(zs), 3))
    x[:, :, 2] = np.repeat(np.asarray(zs, dtype=np.float64), 10)[None, :]
    x[:, :, 0] = 0.25 * np.arange(10 * len(zs))[None, :]
    return dict(top=top, x=x, box=np.tile([4.0, 8.0, LZ], (frames, 1)), lipid_sel=LIPID_SEL, thickness_sel=THICKNESS_SEL,
                exact_tie=True)


def _mixed(n_lipids):
    """Ten-bead and one-bead lipids mixed, a W residue after every third lipid, sides alternating in runs of 1-3."""
    kinds, sides = [], []
    pattern = (1, -1, -1, 1, 1, 1, -1, 1, -1, -1)
    for k in range(n_lipids):
        kinds.append("one" if k % 3 == 1 else "ten")
        sides.append(pattern[k % len(pattern)])
        if k % 3 == 2:
            kinds.append("w")
            sides.append(0)
    return kinds, sides


@functools.lru_cache(maxsize=None)
def get(name: str) -> dict:
    if name == "two":  # one lipid per leaflet
        d = make(["ten", "ten"], [1, -1], 3, seed=1)
    elif name == "single_frame":
        d = make(["ten", "ten", "ten"], [1, -1, 1], 1, seed=2)
    elif name == "sixty_seven":  # 33 / 34, a partial wavefront
        d = make(["ten"] * 67, [1] * 33 + [-1] * 34, 2, seed=3)
    elif name == "mixed300":  # more than one pass of a 256-thread workgroup; lipids of 2 and of 1 selected beads; W between
        kinds, sides = _mixed(300)
        d = make(kinds, sides, 3, seed=4)
    elif name == "seventy_frames":  # a different box in every frame
        d = make(["ten"] * 67, [1] * 33 + [-1] * 34, 70, seed=5, vary_box=True)
    elif name == "flip":  # lipid 2 is up in frames 0 and 2, down in frame 1
        d = make(["ten"] * 6, [1, -1, 1, -1, 1, -1], 3, seed=6, flips=((2, 1),))
    elif name == "no_thickness_bead":  # one-bead lipids own no PO4
        d = make(["ten", "one", "ten", "one", "ten", "ten", "w"], [1, 1, -1, -1, 1, -1, 0], 2, seed=7)
    elif name == "tie":  # midpoint (1 + 3 + 2) / 3 = 2 exactly: the lipid at 2 goes to the lower leaflet
        d = _exact([1.0, 3.0, 2.0])
    elif name == "empty_upper":  # every lipid at the midpoint: all in leaflet -1
        d = _exact([2.0, 2.0, 2.0, 2.0], frames=2)
    else:
        raise KeyError(name)
    top = d["top"]
    ref = R.membrane(d["x"], d["box"], top.residue_index, R.mask(top, ("GL1", "GL2")), R.mask(top, ("PO4",)))
    gap = np.abs(ref["lipid_z"] - ref["mid"][:, None])
    if d["exact_tie"]:
        assert np.all((gap == 0.0) | (gap >= 0.5)), name
    else:
        assert gap.min() > 1e-6, (name, gap.min())
    d["ref"] = ref
    return d


NAMES = ("two", "single_frame", "sixty_seven", "mixed300", "seventy_frames", "flip", "no_thickness_bead", "tie", "empty_upper")
