"""Independent replicas of one system advanced as ONE system: the copies are laid out on a grid far apart in free space,
copy ``r`` owning the nucleotides ``[r * n_one, (r + 1) * n_one)``.  Everything that depends on that layout - the tiled
topology, pair list, external forces and sequence tables, where the copies are put and how trajectory rows and the final
state come apart again - is here.  A layout of one replica hands every input back untouched: no copy, no arithmetic.
"""

from __future__ import annotations

import dataclasses as dc

import numpy as np
import torch


@dc.dataclass(frozen=True)
class ReplicaLayout:
    n_rep: int
    n_one: int  # nucleotides per replica

    def _shifted(self, index, width: int) -> np.ndarray:
        """Rows of nucleotide indices, once per replica, each copy naming its own replica's nucleotides."""
        rows = np.asarray(index).reshape(-1, width)
        return np.concatenate([rows + r * self.n_one for r in range(self.n_rep)], axis=0)

    def topology(self, seq, is_end, bonded, is_rna=None, box=None):
        """(seq, is_end, bonded, is_rna) of all replicas."""
        if self.n_rep == 1:
            return seq, is_end, bonded, is_rna
        if box is not None:
            raise ValueError("HipMDSimulator: replicas are batched in free space; the energy function has a periodic box")
        tile = lambda a: None if a is None else np.tile(np.asarray(a), self.n_rep)  # noqa: E731
        return tile(seq), tile(is_end), self._shifted(bonded, 2), tile(is_rna)

    def pairs(self, pairs):
        return pairs if self.n_rep == 1 else self._shifted(pairs, 2)

    def forces(self, index, force):
        """External forces ``(index (m,), force (m, 3))`` on one replica -> the same on every replica."""
        if self.n_rep == 1:
            return index, force
        return self._shifted(index, 1).reshape(-1), np.tile(force, (self.n_rep, 1))

    def restraint_frames(self, c_init: torch.Tensor, offsets):
        """What restraints need of the layout (Restraints.lower): the initial centres of every replica in its own frame
        (n_rep, n_one, 3) and the translation ``place`` gave each replica (n_rep, 3), both float64 on the host - an anchor
        moves with its replica, the target of a sum by the translation times its number of members."""
        ref = c_init.detach().double().cpu().numpy().reshape(-1, self.n_one, 3)
        ref = np.broadcast_to(ref, (self.n_rep, self.n_one, 3))
        off = np.zeros((self.n_rep, 3)) if offsets is None else offsets.detach().double().cpu().numpy().reshape(self.n_rep, 3)
        return ref, off

    def pseq(self, marg, unit, bp, terms):
        """Sequence tables (pseq_request) with every replica its own copy of the base pairs: base pair ``k`` of replica
        ``r`` is row ``k + n_bp * r``, its two members the units ``2 k + 2 n_bp r`` and ``+ 1``."""
        if self.n_rep == 1:
            return marg, unit, bp, terms
        n_bp = int(bp.shape[0]) if (unit >= 0).any() else 0
        unit = np.concatenate([np.where(unit >= 0, unit + 2 * n_bp * r, -1) for r in range(self.n_rep)])
        return np.tile(marg, (self.n_rep, 1)), unit, (np.tile(bp, (self.n_rep, 1)) if n_bp > 0 else bp), terms

    def place(self, c: torch.Tensor, q: torch.Tensor, r_list: float):
        """Initial state -> (centres (n_rep * n_one, 3), quaternions (n_rep * n_one, 4), offsets) on the grid.  ``c`` (n, 3):
        every replica starts from it; (R, n, 3): one start per replica.  ``r_list``: the range of the neighbour list."""
        if self.n_rep == 1:
            return c, q, None
        n_rep, n_one = self.n_rep, self.n_one
        c = (c if c.dim() == 3 else c[None].expand(n_rep, -1, -1)).reshape(n_rep, n_one, 3).clone()
        q = (q if q.dim() == 3 else q[None].expand(n_rep, -1, -1)).reshape(n_rep, n_one, 4).clone()
        # every replica is centred on its grid node for the run (free space: a translation changes nothing) and gets
        # its own centre of mass back afterwards, so drift accumulated over earlier runs never eats into the spacing
        com = c.mean(dim=1, keepdim=True)
        extent = float((c - com).norm(dim=-1).max())
        spacing = 2.0 * extent + 8.0 * r_list + 64.0  # out of each other's list range for as long as a run diffuses
        side = int(np.ceil(n_rep ** (1.0 / 3.0)))
        grid = torch.as_tensor([[r % side, (r // side) % side, r // (side * side)] for r in range(n_rep)], dtype=c.dtype, device=c.device)
        offsets = (grid * spacing)[:, None, :] - com
        return (c + offsets).reshape(n_rep * n_one, 3).contiguous(), q.reshape(n_rep * n_one, 4).contiguous(), offsets

    def unplace_rows(self, tc, tq, et, offsets):
        """Saved rows (S, n_rep * n_one, .) -> the states of all replicas, replica-major (n_rep * S, n_one, .), in their own
        frames.  The fused energy trace sums over the whole launch, so replicas have none: per-replica energies come from
        the energy function."""
        if self.n_rep == 1:
            return tc, tq, et

        def unbatch(t, width, off):
            t = t.reshape(t.shape[0], self.n_rep, self.n_one, width)
            if off is not None:
                t = t - off[None]
            return t.transpose(0, 1).reshape(-1, self.n_one, width)

        return (None if tc is None else unbatch(tc, 3, offsets)), (None if tq is None else unbatch(tq, 4, None)), None

    def unplace_state(self, c, q, offsets):
        """The stepped state -> (n_rep, n_one, .) in the replicas' own frames."""
        if self.n_rep == 1:
            return c, q
        return c.reshape(self.n_rep, self.n_one, 3) - offsets, q.reshape(self.n_rep, self.n_one, 4)
