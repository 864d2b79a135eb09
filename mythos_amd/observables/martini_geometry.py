"""What the MARTINI bond-length and triplet-angle observables share: name matching and the one HIP launch that
evaluates every selected group for every frame (mythos_amd/csrc/martini_obs.hip, ``mythos_martini_obs_eval``).

A group is every bond (or angle) of the topology that carries one name.  The launch writes a packed float64 block,
group-major: group g with m_g members is the (S, m_g) row-major block at S * (m_0 + ... + m_{g-1}) - the layout
``WassersteinDistanceMapped`` builds its plan from.
"""

from __future__ import annotations

import numpy as np
import torch

from mythos_amd import _lib
from mythos_amd.hip_system import martini_frames


def matching(all_names, name: str, kind: str) -> list[int]:
    """Indices of the topology's bonds / angles called ``name``; the reference's error otherwise
    (mythos/observables/bond_distances.py:41-49, triplet_angles.py:64-71)."""
    idx = [i for i, n in enumerate(all_names) if n == name]
    if not idx:
        raise ValueError(f"No {kind}s matching '{name}' found in the topology. Available {kind} names: {sorted(set(all_names))}")
    return idx


class GeometrySet(_lib.Handle):
    """mythos_martini_obs_t: the index lists of some groups on one device."""

    _destroy = "mythos_martini_obs_destroy"

    def __init__(self, n: int, widths, index_lists, device):
        self.device = torch.device(device)
        self.members = [int(len(ix)) for ix in index_lists]
        w = np.ascontiguousarray(widths, dtype=np.int32)
        m = np.ascontiguousarray(self.members, dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(ix, dtype=np.int32).reshape(-1) for ix in index_lists]), dtype=np.int32)
        super().__init__("mythos_martini_obs_create", int(n), len(self.members), w.ctypes.data_as(_lib.c_int_p),
                         m.ctypes.data_as(_lib.c_int_p), flat.ctypes.data_as(_lib.c_int_p), self.device.index or 0)
        self.count = int(self._lib.mythos_martini_obs_count(self._h))

    def eval(self, pos: torch.Tensor, box: torch.Tensor) -> torch.Tensor:
        """The packed (S * count,) float64 block of (S, n, 3) positions and (S, 3) boxes of one dtype."""
        s = int(pos.shape[0])
        out = torch.empty(s * self.count, dtype=torch.float64, device=self.device)
        _lib.check(self._lib.mythos_martini_obs_eval(self._h, _lib.ptr(pos), _lib.ptr(box), _lib.dtype_code(pos.dtype), s, _lib.ptr(out),
                                                     _lib.stream(self.device)), "martini_obs_eval")
        return out


class MappedGeometry:
    """Base of the ``*Mapped`` observables: ``names`` -> dict of (S, n_matching) float64 device tensors, one launch.

    Only the per-frame orthorhombic periodic displacement (``trajectory.box_size``) is supported - what the MARTINI
    energy kernels support; there is no ``displacement_fn`` argument."""

    kind = "bond"
    width = 2

    def _all_names(self):
        raise NotImplementedError

    def _all_index(self):
        raise NotImplementedError

    @property
    def names(self) -> tuple:
        raise NotImplementedError

    def index_lists(self) -> list:
        """Per name the (n_matching, width) bead indices; raises the reference's ValueError for an unknown name."""
        cached = self.__dict__.get("_index_lists")
        if cached is None:
            all_names, index = self._all_names(), np.asarray(self._all_index())
            cached = [index[matching(all_names, n, self.kind)] for n in self.names]
            self.__dict__["_index_lists"] = cached
        return cached

    def packed(self, trajectory):
        """(block, S, members): the packed block of the launch and its layout."""
        lists = self.index_lists()
        pos, box = martini_frames(trajectory.center, getattr(trajectory, "box_size", None))
        if pos.shape[1] != len(self.topology.atom_names):
            raise ValueError(f"trajectory has {pos.shape[1]} beads, the topology {len(self.topology.atom_names)}")
        gs = _lib.per_device(self, pos.device, lambda: GeometrySet(int(pos.shape[1]), [self.width] * len(lists), lists, pos.device))
        return gs.eval(pos, box), int(pos.shape[0]), gs.members

    def __call__(self, trajectory) -> dict:
        block, s, members = self.packed(trajectory)
        out, at = {}, 0
        for name, m in zip(self.names, members):
            out[name] = block[at:at + s * m].view(s, m)
            at += s * m
        return out
