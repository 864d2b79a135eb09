"""Angles of named MARTINI bead triplets (mythos/observables/triplet_angles.py:34-136), evaluated by the HIP library:
the angle at the middle bead of (i, j, k), atan2(|r_ij x r_kj|, r_ij . r_kj) on unit vectors as
mythos/energy/martini/m2/angle.py:35-58, minimum image under each frame's orthorhombic box, in double whatever the
dtype of the positions.

    obs = TripletAnglesMapped(topology=top, angle_names=("DMPC_PO4_GL1_GL2",))
    angles = obs(trajectory)             # {name: (S, n_matching) float64 device tensor} in radians, one launch

Only the per-frame periodic displacement of ``trajectory.box_size`` is supported (what the MARTINI energy kernels
support); a trajectory without ``box_size`` raises ``ValueError``.
"""

from __future__ import annotations

import dataclasses as dc

import torch

from mythos_amd.input.gromacs import MartiniTopology
from mythos_amd.observables.martini_geometry import MappedGeometry


@dc.dataclass(frozen=True, kw_only=True)
class TripletAnglesMapped(MappedGeometry):
    topology: MartiniTopology
    angle_names: tuple

    kind = "angle"
    width = 3

    @property
    def names(self) -> tuple:
        return tuple(self.angle_names)

    def _all_names(self):
        return self.topology.angle_names

    def _all_index(self):
        return self.topology.angles


@dc.dataclass(frozen=True, kw_only=True)
class TripletAngles(TripletAnglesMapped):
    """One angle name -> (S, n_matching) tensor."""

    angle_name: str
    angle_names: tuple = ()

    @property
    def names(self) -> tuple:
        return (self.angle_name,)

    def __call__(self, trajectory) -> torch.Tensor:
        return MappedGeometry.__call__(self, trajectory)[self.angle_name]
