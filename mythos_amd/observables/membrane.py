"""Membrane thickness and area per lipid of a bilayer (mythos/observables/membrane_thickness.py:12-43,
area_per_lipid.py:13-41), evaluated by the HIP library in one launch over the stored frames
(mythos_amd/csrc/membrane.hip, ``mythos_membrane_eval``).

    thickness = MembraneThickness(topology=top, lipid_sel="name GL1 GL2", thickness_sel="name PO4")(trajectory)  # (S,) A
    area = AreaPerLipid(topology=top, lipid_sel="name GL1 GL2")(trajectory)                                       # (S,) A^2

The reference computes both through MDAnalysis and LiPyphilic (AssignLeaflets, MembThickness, AreaPerLipid at their
defaults, ``n_bins = 1``).  What those do is restated here and reproduces the ten known answers of
the reference's tests:

* a lipid is a residue that owns at least one bead of ``lipid_sel``; its position is the UNWEIGHTED mean z of those
  beads.  LiPyphilic weights by mass; a ``MartiniTopology`` holds no masses, and for selections of equal-mass beads (the
  reference's ``name GL1 GL2``) the two agree.
* the midpoint of a frame is the mean z of all ``lipid_sel`` beads (over beads, not over lipids); leaflet +1 is
  z_lipid > midpoint, -1 otherwise (a tie goes to -1).
* thickness = mean z of the ``thickness_sel`` beads of leaflet +1 minus that of leaflet -1.  Coordinates are used as
  stored, with no re-wrapping in z: a bilayer that straddles the z boundary of the box is not handled, and what LiPyphilic
  does there is unverified.
* area per lipid of a frame = Lx Ly (occupied leaflets) / n_lipids - the mean over lipids of the Voronoi areas of a
  periodic tessellation, whose cells tile the box, without building the tessellation.  Per-lipid areas do not exist here.
* a frame with an empty leaflet, or a leaflet without a thickness bead, has NaN thickness (this package's definition;
  LiPyphilic's behaviour there is unverified).

Positions are nm as everywhere in this package; results are handed out in the reference's units (MDAnalysis converts):
A and A^2.  ``topology`` is a ``MartiniTopology`` with ``residue_index``; selections are the subset of MDAnalysis'
language that the reference's example and tests use: ``name A B ...``, ``resname R ...``, the two joined by ``and``, or a
tuple of bead names.
"""

from __future__ import annotations

import dataclasses as dc
import re

import numpy as np
import torch

from mythos_amd import _lib
from mythos_amd.hip_system import martini_frames
from mythos_amd.input.gromacs import MartiniTopology

ANGSTROM_PER_NM = 10.0
_FIELDS = {"name": "atom_names", "resname": "residue_names"}
_NAME = re.compile(r"[A-Za-z0-9_+\-']+")
# words of MDAnalysis' selection language that are not bead or residue names
_KEYWORDS = frozenset("and or not all none around sphlayer sphzone cylayer cyzone point prop resid resnum index bynum type segid "
                      "byres same as global group bonded protein nucleic backbone moltype molnum mass charge altloc icode "
                      "chainid element within isolayer".split())


def select(topology: MartiniTopology, selection) -> np.ndarray:
    """Boolean mask over beads of ``name A B ...`` / ``resname R ...`` / their ``and`` / a tuple of bead names."""
    n = len(topology.atom_names)
    if not isinstance(selection, str):
        wanted = {str(a) for a in selection}
        mask = np.array([a in wanted for a in topology.atom_names], dtype=bool)
    else:
        mask, field, values = np.ones(n, dtype=bool), None, []

        def close():
            nonlocal mask
            if field is None or not values:
                raise ValueError(f"selection {selection!r}: expected 'name A B ...' or 'resname R ...' (joined by 'and')")
            mask &= np.isin(np.asarray(getattr(topology, _FIELDS[field])), values)

        for tok in selection.split():
            if tok in _FIELDS and field is None:
                field = tok
            elif tok == "and" and values:
                close()
                field, values = None, []
            elif field is not None and _NAME.fullmatch(tok) and tok not in _KEYWORDS and tok not in _FIELDS:
                values.append(tok)
            else:
                raise ValueError(f"selection {selection!r}: unsupported token {tok!r} (supported: 'name A B ...', "
                                 "'resname R ...', the two joined by 'and')")
        close()
    if not mask.any():
        raise ValueError(f"selection {selection!r} matches no bead of the topology")
    return mask


class MembraneSet(_lib.Handle):
    """mythos_membrane_t: the index lists of one pair of selections on one device."""

    _destroy = "mythos_membrane_destroy"

    def __init__(self, n, start, sel, thick, thick_lipid, device):
        self.device = torch.device(device)
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (start, sel, thick, thick_lipid)]
        super().__init__("mythos_membrane_create", int(n), len(arrs[0]) - 1, arrs[0].ctypes.data_as(_lib.c_int_p),
                         arrs[1].ctypes.data_as(_lib.c_int_p), len(arrs[2]), arrs[2].ctypes.data_as(_lib.c_int_p),
                         arrs[3].ctypes.data_as(_lib.c_int_p), self.device.index or 0)
        self.n_lipids = int(self._lib.mythos_membrane_n_lipids(self._h))

    def eval(self, pos: torch.Tensor, box: torch.Tensor, want_leaflets: bool = False):
        """-> ((S, MEMBRANE_ROW) float64 rows, (S, n_lipids) int8 leaflets or None)."""
        s = int(pos.shape[0])
        out = torch.empty((s, _lib.MEMBRANE_ROW), dtype=torch.float64, device=self.device)
        leaf = torch.empty((s, self.n_lipids), dtype=torch.int8, device=self.device) if want_leaflets else None
        _lib.check(self._lib.mythos_membrane_eval(self._h, _lib.ptr(pos), _lib.ptr(box), _lib.dtype_code(pos.dtype), s, _lib.ptr(out),
                                                  _lib.ptr(leaf), _lib.stream(self.device)), "membrane_eval")
        return out, leaf


class _Membrane:
    """What MembraneThickness and AreaPerLipid share: the index lists and the launch."""

    thickness_sel = None

    def index_lists(self):
        """(lipid_residues, start, sel, thick, thick_lipid), built once; the ValueErrors of the selections."""
        cached = self.__dict__.get("_lists")
        if cached is None:
            top = self.topology
            if getattr(top, "residue_index", None) is None:
                raise ValueError("membrane observables need topology.residue_index (MartiniTopology.from_top / from_tpr fill it)")
            resid = np.asarray(top.residue_index)
            beads = np.flatnonzero(select(top, self.lipid_sel))
            residues, lipid_of = np.unique(resid[beads], return_inverse=True)
            order = np.argsort(lipid_of, kind="stable")  # group by lipid, bead order kept inside a lipid
            start = np.concatenate([[0], np.cumsum(np.bincount(lipid_of, minlength=len(residues)))])
            thick = np.zeros(0, dtype=np.int64)
            thick_lipid = thick
            if self.thickness_sel is not None:
                thick = np.flatnonzero(select(top, self.thickness_sel))
                thick_lipid = np.searchsorted(residues, resid[thick])
                stray = (thick_lipid >= len(residues)) | (residues[np.minimum(thick_lipid, len(residues) - 1)] != resid[thick])
                if stray.any():
                    b = int(thick[np.argmax(stray)])
                    raise ValueError(f"thickness_sel bead {b} ({top.residue_names[b]} {top.atom_names[b]}, residue {int(resid[b])}) "
                                     f"is in a residue with no bead of lipid_sel {self.lipid_sel!r}")
            cached = (residues.astype(np.int64), start, beads[order], thick, thick_lipid)
            self.__dict__["_lists"] = cached
        return cached

    @property
    def lipid_residues(self) -> np.ndarray:
        """``residue_index`` of the lipids, in the order of the columns of ``leaflets``."""
        return self.index_lists()[0]

    def _rows(self, trajectory, want_leaflets=False):
        lists = self.index_lists()
        pos, box = martini_frames(trajectory.center, getattr(trajectory, "box_size", None))
        if pos.shape[1] != len(self.topology.atom_names):
            raise ValueError(f"trajectory has {pos.shape[1]} beads, the topology {len(self.topology.atom_names)}")
        return _lib.per_device(self, pos.device, lambda: MembraneSet(int(pos.shape[1]), *lists[1:], pos.device)).eval(pos, box, want_leaflets)

    def rows(self, trajectory) -> torch.Tensor:
        """The launch's (S, 7) float64 rows in nm: thickness, area per lipid, midpoint z, lipids in leaflet +1 and -1,
        mean z of the thickness beads of leaflet +1 and -1."""
        return self._rows(trajectory)[0]

    def leaflets(self, trajectory) -> torch.Tensor:
        """(S, n_lipids) int8: +1 / -1 per lipid and frame."""
        return self._rows(trajectory, want_leaflets=True)[1]


@dc.dataclass(frozen=True, kw_only=True)
class MembraneThickness(_Membrane):
    """(S,) float64 device tensor, Angstrom; NaN for a frame with an empty leaflet."""

    topology: MartiniTopology
    lipid_sel: str | tuple
    thickness_sel: str | tuple

    def __call__(self, trajectory) -> torch.Tensor:
        return self.rows(trajectory)[:, 0] * ANGSTROM_PER_NM


@dc.dataclass(frozen=True, kw_only=True)
class AreaPerLipid(_Membrane):
    """(S,) float64 device tensor, Angstrom^2: the frame's mean over lipids."""

    topology: MartiniTopology
    lipid_sel: str | tuple

    def __call__(self, trajectory) -> torch.Tensor:
        return self.rows(trajectory)[:, 1] * (ANGSTROM_PER_NM * ANGSTROM_PER_NM)
