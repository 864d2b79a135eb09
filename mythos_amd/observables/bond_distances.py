"""Bond lengths of named MARTINI bonds (mythos/observables/bond_distances.py:20-113), evaluated by the HIP library:
|minimum image of x_i - x_j| under each frame's orthorhombic box, in double whatever the dtype of the positions.

    obs = BondDistancesMapped(topology=top, bond_names=("DMPC_NC3_PO4", "DMPC_GL1_GL2"))
    lengths = obs(trajectory)            # {name: (S, n_matching) float64 device tensor}, one launch for all names

Only the per-frame periodic displacement of ``trajectory.box_size`` is supported (what the MARTINI energy kernels
support): the reference's ``displacement_fn`` argument does not exist here, and a trajectory without ``box_size``
raises ``ValueError``.
"""

from __future__ import annotations

import dataclasses as dc

import torch

from mythos_amd.input.gromacs import MartiniTopology
from mythos_amd.observables.martini_geometry import MappedGeometry


@dc.dataclass(frozen=True, kw_only=True)
class BondDistancesMapped(MappedGeometry):
    topology: MartiniTopology
    bond_names: tuple

    kind = "bond"
    width = 2

    @property
    def names(self) -> tuple:
        return tuple(self.bond_names)

    def _all_names(self):
        return self.topology.bond_names

    def _all_index(self):
        return self.topology.bonded_neighbors


@dc.dataclass(frozen=True, kw_only=True)
class BondDistances(BondDistancesMapped):
    """One bond name -> (S, n_matching) tensor."""

    bond_name: str
    bond_names: tuple = ()

    @property
    def names(self) -> tuple:
        return (self.bond_name,)

    def __call__(self, trajectory) -> torch.Tensor:
        return MappedGeometry.__call__(self, trajectory)[self.bond_name]
