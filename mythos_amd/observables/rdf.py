"""Radial distribution functions g(r) between selections of MARTINI beads, of every stored frame, evaluated by the HIP
library in one launch for all named pairs (mythos_amd/csrc/rdf.hip, ``mythos_rdf_eval``).

    rdf = RadialDistribution(topology=top, pairs={"PO4-PO4": ("name PO4", "name PO4"), "PO4-tail": ("name PO4", "name C3A C3B")},
                             r_max=2.0, n_bins=200, exclude="residue", dims="xyz")
    g = rdf(trajectory)          # {name: (F, n_bins) float64 on the GPU}; one launch for all names
    c = rdf.counts(trajectory)   # {name: (F, n_bins) int64}
    rdf.r, rdf.edges, rdf.n_pairs[name]          # bin centres, bin edges (numpy), admissible ordered pairs
    expected = weights @ g["PO4-PO4"]            # the reweighted RDF of DiffTRe; differentiable in the weights

Definitions.  For a pair of selections A, B every ORDERED pair (i in A, j in B) with i != j - and,
under ``exclude="residue"``, with different ``topology.residue_index``: no intramolecular pairs, MDAnalysis'
``exclusion_block`` - whose minimum-image distance r under the frame's own orthorhombic box is below ``r_max`` adds 1 to
bin ``floor(r n_bins / r_max)``.  A and B may be the same selection, disjoint or overlapping.  ``dims="xy"`` measures r
and takes the minimum image in x and y alone: the lateral RDF of a membrane (both leaflets together).  Arithmetic is
double whatever the dtype of the positions; the counts are integers and have the same bits from run to run.

Normalisation is per frame, with the frame's own box, so frames of an NPT run are right:

    g[f, b] = counts[f, b] V_f / (N_pairs v_b)

with V_f = Lx Ly Lz and v_b = 4 pi / 3 (r_{b+1}^3 - r_b^3) for ``xyz``, V_f = Lx Ly and v_b = pi (r_{b+1}^2 - r_b^2) for
``xy``, and N_pairs the number of admissible ordered pairs - |A| |B| minus the pairs with i = j minus the pairs that
share a block - computed once on the host.  This is MDAnalysis ``InterRDF(norm="rdf")`` with each frame's own volume in
place of the run's mean volume; ``counts`` is there for whoever wants another convention.

``r_max`` may not exceed half the shortest box edge (of x and y for ``xy``) of any frame: beyond that the minimum image
does not find the closest pair.  The kernel reports the first frame that breaks this and the call raises ``ValueError``
naming it.  Reading that word back is one host synchronisation per call.

Limit: brute force over the two selections, F |A| |B| distances per pair of selections, no cell list.  That is the
design at the sizes this package stores (1 280 to about 20 000 beads, hundreds of frames); a selection holds at most
2^22 beads and ``n_bins`` is at most 4096.  Selections are those of ``observables.membrane.select``.
"""

from __future__ import annotations

import ctypes as C
import dataclasses as dc
import math

import numpy as np
import torch

from mythos_amd import _lib
from mythos_amd.hip_system import martini_frames
from mythos_amd.input.gromacs import MartiniTopology
from mythos_amd.observables.membrane import select

MAX_BINS = 4096
_DIMS = {"xy": 2, "xyz": 3}  # MYTHOS_RDF_XY, MYTHOS_RDF_XYZ of include/mythos_hip.h


def admissible_pairs(a, b, block=None) -> int:
    """Ordered pairs (i in a, j in b) with i != j and, where ``block`` (an id per bead) is given, block[i] != block[j]."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    ids_a, ids_b = (a, b) if block is None else (np.asarray(block)[a], np.asarray(block)[b])
    ua, ca = np.unique(ids_a, return_counts=True)
    ub, cb = np.unique(ids_b, return_counts=True)
    _, ia, ib = np.intersect1d(ua, ub, assume_unique=True, return_indices=True)
    return int(len(a)) * int(len(b)) - int((ca[ia].astype(np.int64) * cb[ib].astype(np.int64)).sum())


def shell_volumes(edges, dims: str = "xyz") -> np.ndarray:
    """v_b of the normalisation: volumes of the spherical shells (``xyz``) or areas of the rings (``xy``) between edges."""
    e = np.asarray(edges, dtype=np.float64)
    if dims == "xyz":
        return 4.0 * math.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3)
    if dims == "xy":
        return math.pi * (e[1:] ** 2 - e[:-1] ** 2)
    raise ValueError(f"dims {dims!r}: expected 'xyz' or 'xy'")


class _RdfSet(_lib.Handle):
    """mythos_rdf_t: the bead lists of some pairs of selections, the blocks and the bins on one device.  Private: the
    observables below are the interface (tests/test_gpu_api.py lists the public owners of a handle; this one's close() is
    tested with the kernel's own tests)."""

    _destroy = "mythos_rdf_destroy"

    def __init__(self, n, lists, block, n_bins, r_max, dims, device):
        self.device = torch.device(device)
        self.n_groups, self.n_bins = len(lists), int(n_bins)
        n_a = np.ascontiguousarray([len(a) for a, _ in lists], dtype=np.int32)
        n_b = np.ascontiguousarray([len(b) for _, b in lists], dtype=np.int32)
        index = np.ascontiguousarray(np.concatenate([np.concatenate([a, b]) for a, b in lists]), dtype=np.int32)
        blk = None if block is None else np.ascontiguousarray(block, dtype=np.int32)
        super().__init__("mythos_rdf_create", int(n), self.n_groups, n_a.ctypes.data_as(_lib.c_int_p), n_b.ctypes.data_as(_lib.c_int_p),
                         index.ctypes.data_as(_lib.c_int_p), None if blk is None else blk.ctypes.data_as(_lib.c_int_p), self.n_bins,
                         float(r_max), _DIMS[dims], self.device.index or 0)
        pairs = (C.c_int64 * self.n_groups)()
        _lib.check(self._lib.mythos_rdf_n_pairs(self._h, pairs), "rdf_n_pairs")
        self.n_pairs = [int(p) for p in pairs]

    def launch(self, pos: torch.Tensor, box: torch.Tensor):
        """-> ((F, n_groups, n_bins) int64 counts, (1,) int32 flag) on the device, nothing read back: the flag is -1, or the
        first frame with an edge of a masked dimension below 2 r_max."""
        f = int(pos.shape[0])
        counts = torch.empty((f, self.n_groups, self.n_bins), dtype=torch.int64, device=self.device)
        flag = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(self._lib.mythos_rdf_eval(self._h, _lib.ptr(pos), _lib.ptr(box), _lib.dtype_code(pos.dtype), f, _lib.ptr(counts),
                                             _lib.ptr(flag), _lib.stream(self.device)), "rdf_eval")
        return counts, flag

    def eval(self, pos: torch.Tensor, box: torch.Tensor):
        """-> (counts, the flag as an int): reading it is one host synchronisation."""
        counts, flag = self.launch(pos, box)
        return counts, int(flag.item())


class _Rdf:
    """What RadialDistribution and RadialDistributionPair share: the plan on the host, the launch, the normalisation."""

    def _pairs(self) -> dict:
        raise NotImplementedError

    def __post_init__(self):
        self.plan()  # the ValueErrors of the arguments and selections, where the object is made

    def plan(self):
        """(names, [(A, B) bead index arrays], block or None, {name: N_pairs}), built once on the host."""
        cached = self.__dict__.get("_plan")
        if cached is None:
            top, pairs = self.topology, self._pairs()
            if self.dims not in _DIMS:
                raise ValueError(f"dims {self.dims!r}: expected 'xyz' or 'xy'")
            if int(self.n_bins) != self.n_bins or not 1 <= self.n_bins <= MAX_BINS:
                raise ValueError(f"n_bins {self.n_bins!r}: expected an integer in [1, {MAX_BINS}]")
            if not (self.r_max > 0.0 and math.isfinite(self.r_max)):
                raise ValueError(f"r_max {self.r_max!r}: expected a positive length")
            if self.exclude not in (None, "residue"):
                raise ValueError(f"exclude {self.exclude!r}: expected 'residue' or None")
            block = None
            if self.exclude == "residue":
                if getattr(top, "residue_index", None) is None:
                    raise ValueError("exclude='residue' needs topology.residue_index (MartiniTopology.from_top / from_tpr fill it)")
                block = np.asarray(top.residue_index, dtype=np.int64)
            if not pairs:
                raise ValueError("pairs: expected at least one name -> (selection A, selection B)")
            lists, n_pairs = [], {}
            for name, sels in pairs.items():
                if isinstance(sels, str) or len(sels) != 2:
                    raise ValueError(f"pair {name!r}: expected (selection A, selection B)")
                a, b = (np.flatnonzero(select(top, s)) for s in sels)
                n_pairs[name] = admissible_pairs(a, b, block)
                if n_pairs[name] == 0:
                    why = "is the same bead" if block is None else "is the same bead or shares a residue"
                    raise ValueError(f"pair {name!r}: no admissible pair of beads (every pair of {sels[0]!r} and {sels[1]!r} {why})")
                lists.append((a, b))
            cached = (tuple(pairs), lists, block, n_pairs)
            self.__dict__["_plan"] = cached
        return cached

    @property
    def names(self) -> tuple:
        return self.plan()[0]

    @property
    def n_pairs(self) -> dict:
        """{name: admissible ordered pairs}: the N_pairs of the normalisation."""
        return dict(self.plan()[3])

    @property
    def edges(self) -> np.ndarray:
        """(n_bins + 1,) bin edges, 0 ... r_max."""
        return np.linspace(0.0, float(self.r_max), int(self.n_bins) + 1)

    @property
    def r(self) -> np.ndarray:
        """(n_bins,) bin centres."""
        e = self.edges
        return 0.5 * (e[1:] + e[:-1])

    @property
    def shell_volumes(self) -> np.ndarray:
        return shell_volumes(self.edges, self.dims)

    def _launch(self, trajectory):
        names, lists, block, _ = self.plan()
        pos, box = martini_frames(trajectory.center, getattr(trajectory, "box_size", None))
        if pos.shape[1] != len(self.topology.atom_names):
            raise ValueError(f"trajectory has {pos.shape[1]} beads, the topology {len(self.topology.atom_names)}")
        rs = _lib.per_device(self, pos.device, lambda: _RdfSet(int(pos.shape[1]), lists, block, self.n_bins, self.r_max, self.dims, pos.device))
        counts, short = rs.eval(pos, box)
        if short >= 0:
            edges = "x, y" if self.dims == "xy" else "x, y, z"
            raise ValueError(f"frame {short}: a box edge ({edges}) is shorter than 2 r_max = {2.0 * float(self.r_max)}; "
                             "the minimum image does not find the closest pair there")
        return counts, box

    def counts(self, trajectory) -> dict:
        """{name: (F, n_bins) int64 device tensor}: the ordered pairs per bin and frame.  One launch for all names, one
        host synchronisation for the r_max check."""
        counts, _ = self._launch(trajectory)
        return {name: counts[:, g] for g, name in enumerate(self.names)}

    def __call__(self, trajectory) -> dict:
        """{name: (F, n_bins) float64 device tensor} g(r), normalised per frame (module docstring).  One launch for all
        names, one host synchronisation for the r_max check."""
        counts, box = self._launch(trajectory)
        box = box.to(torch.float64)
        volume = box[:, 0] * box[:, 1] * (box[:, 2] if self.dims == "xyz" else 1.0)
        shells = torch.as_tensor(self.shell_volumes, device=counts.device)
        n_pairs = self.plan()[3]
        return {name: counts[:, g].to(torch.float64) * volume[:, None] / (float(n_pairs[name]) * shells)[None, :]
                for g, name in enumerate(self.names)}


@dc.dataclass(frozen=True, kw_only=True)
class RadialDistribution(_Rdf):
    """``pairs``: {name: (selection A, selection B)} -> {name: (F, n_bins)} g(r); see the module docstring."""

    topology: MartiniTopology
    pairs: dict
    r_max: float
    n_bins: int
    exclude: str | None = None
    dims: str = "xyz"

    def _pairs(self) -> dict:
        return dict(self.pairs)


@dc.dataclass(frozen=True, kw_only=True)
class RadialDistributionPair(_Rdf):
    """One pair of selections -> the (F, n_bins) tensor itself."""

    topology: MartiniTopology
    sel_a: str | tuple
    sel_b: str | tuple
    r_max: float
    n_bins: int
    exclude: str | None = None
    dims: str = "xyz"

    def _pairs(self) -> dict:
        return {"pair": (self.sel_a, self.sel_b)}

    def counts(self, trajectory) -> torch.Tensor:
        return _Rdf.counts(self, trajectory)["pair"]

    def __call__(self, trajectory) -> torch.Tensor:
        return _Rdf.__call__(self, trajectory)["pair"]
