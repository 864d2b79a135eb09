"""Oracle-side reference of oxDNA's ``bond`` and ``mindistance`` order parameters, and the inputs the order-parameter
tests share.

Per-pair rows: the CPU oracle's ``pair_terms`` with the LISTED pairs (lower index first, the reference's i < j) as its
unbonded list gives the hydrogen-bonding energy of every listed pair; ``orc.Sites`` gives the base sites whose
minimum-image distance is the ``mindistance`` row.  The frames of a trajectory are stacked into one system of F x N
nucleotides (the trick of tests/melting_ref.oracle_frame_terms).  States: the count of energies strictly below the
cutoff, and the number of interfaces the smallest distance strictly exceeds.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

from mythos_amd.input.order_parameters import OrderParameter, read_order_parameters
from oracle import oxdna_oracle as orc
from tests import helpers as H
from tests import melting_ref as M

HB_CUTOFF = -0.1
OP_FILE = M.FIXTURE / "op.txt"


def sorted_pairs(pairs) -> np.ndarray:
    return np.sort(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), axis=1)


def oracle_rows(model, P, seq, center, quat, pairs, box=None):
    """(hb (F, P), dist (F, P)) float64 numpy: hydrogen-bonding energy and base-base distance of the listed pairs."""
    center = torch.as_tensor(np.asarray(center), dtype=torch.float64)
    quat = torch.as_tensor(np.asarray(quat), dtype=torch.float64)
    if center.dim() == 2:
        center, quat = center[None], quat[None]
    nf, n = center.shape[0], center.shape[1]
    pr = torch.as_tensor(sorted_pairs(pairs))
    off = (torch.arange(nf) * n)[:, None, None]
    stacked = (pr[None] + off).reshape(-1, 2)
    seq_t = torch.as_tensor(np.asarray(seq), dtype=torch.long).repeat(nf)
    c, q = center.reshape(-1, 3), quat.reshape(-1, 4)
    box_t = None if box is None else np.broadcast_to(np.asarray(box, dtype=np.float64), (3,)).copy()
    _, ut = orc.pair_terms(model, P, c, q, seq_t, torch.zeros(nf * n, dtype=torch.long), torch.zeros((0, 2), dtype=torch.long),
                           stacked, box=box_t)
    a1, a2, a3 = orc.quat_to_axes(q)
    sites = orc.Sites(model, P["geometry"], c, a1, a2, a3)
    d = orc.make_displacement(box_t)(sites.base[stacked[:, 1]], sites.base[stacked[:, 0]])
    dist = torch.sqrt((d * d).sum(-1))
    return ut["hydrogen_bonding"].detach().reshape(nf, -1).numpy(), dist.detach().reshape(nf, -1).numpy()


def site_distance(model, P, center, quat, pairs, site: str, box=None) -> np.ndarray:
    """(F, P) minimum-image distance between another site of the listed pairs (``center``, ``back``, ``stack``, ``base``):
    what the fixture's ``mindistance`` column is NOT, except for ``base``."""
    center = torch.as_tensor(np.asarray(center), dtype=torch.float64)
    quat = torch.as_tensor(np.asarray(quat), dtype=torch.float64)
    nf, n = center.shape[0], center.shape[1]
    c, q = center.reshape(-1, 3), quat.reshape(-1, 4)
    a1, a2, a3 = orc.quat_to_axes(q)
    s = getattr(orc.Sites(model, P["geometry"], c, a1, a2, a3), site)
    pr = torch.as_tensor(sorted_pairs(pairs))
    stacked = (pr[None] + (torch.arange(nf) * n)[:, None, None]).reshape(-1, 2)
    box_t = None if box is None else np.broadcast_to(np.asarray(box, dtype=np.float64), (3,)).copy()
    d = orc.make_displacement(box_t)(s[stacked[:, 1]], s[stacked[:, 0]])
    return torch.sqrt((d * d).sum(-1)).reshape(nf, -1).numpy()


def slices(ops):
    first = np.concatenate([[0], np.cumsum([len(o.pairs) for o in ops])])
    return [(int(first[k]), int(first[k + 1])) for k in range(len(ops))]


def all_pairs(ops) -> np.ndarray:
    return np.asarray([p for o in ops for p in o.pairs], dtype=np.int64).reshape(-1, 2)


def values_from_rows(hb, dist, ops, cutoff=HB_CUTOFF) -> np.ndarray:
    """(F, n_ops) float64: bond count / smallest distance from the (F, P) rows of all the ops' pairs back to back."""
    cols = []
    for o, (a, b) in zip(ops, slices(ops)):
        cols.append((hb[:, a:b] < cutoff).sum(1).astype(np.float64) if o.kind == "bond" else dist[:, a:b].min(1))
    return np.stack(cols, axis=1)


def states_from_values(values, ops) -> np.ndarray:
    cols = []
    for k, o in enumerate(ops):
        v = values[:, k]
        cols.append(np.rint(v).astype(np.int64) if o.kind == "bond"
                    else (v[:, None] > np.asarray(o.interfaces)[None, :]).sum(1).astype(np.int64))
    return np.stack(cols, axis=1)


def states_from_rows(hb, dist, ops, cutoff=HB_CUTOFF) -> np.ndarray:
    return states_from_values(values_from_rows(hb, dist, ops, cutoff), ops)


def near_cutoff(hb, bound, cutoff=HB_CUTOFF) -> np.ndarray:
    """(F, P) bool: entries whose oracle energy lies within ``bound`` of the cutoff - where a kernel that is right to
    ``bound`` may still land on the other side."""
    return np.abs(hb - cutoff) <= bound


@functools.lru_cache(maxsize=None)
def golden_ops():
    return read_order_parameters(OP_FILE)


@functools.lru_cache(maxsize=None)
def golden_rows():
    """dna1 defaults, periodic box 20, all 384 frames of tests/golden/melting_temp: (ops, hb (384, 12), dist (384, 12),
    energy-file columns) - computed once, read-only."""
    top, traj, en = M.load_run()
    ops = golden_ops()
    P = H.oracle_params(1)
    hb, dist = oracle_rows(1, P, top.seq, traj.center, traj.quaternions, all_pairs(ops), box=M.BOX)
    hb.setflags(write=False)
    dist.setflags(write=False)
    return ops, hb, dist, en


def weight_table(en, names=("bond", "mindistance")) -> dict:
    """{state tuple: weight} from the distinct (state -> weight) rows of an energy file's columns."""
    st = np.stack([en[n] for n in names], axis=1).astype(np.int64)
    table = {}
    for row, w in zip(st, en["weight"]):
        key = tuple(int(x) for x in row)
        assert table.setdefault(key, float(w)) == float(w), f"state {key} carries two weights"
    return table


def native_ops(n_bp: int, n: int | None = None, kinds=("bond", "mindistance"), interfaces=(1.0, 2.0, 4.0)):
    """Order parameters over the native pairs (k, n - 1 - k) of an n_bp-bp duplex of n = 2 n_bp nucleotides."""
    n = 2 * n_bp if n is None else n
    pairs = tuple((k, n - 1 - k) for k in range(n_bp))
    return tuple(OrderParameter(kind=kd, name=f"{kd}_{k}", pairs=pairs, interfaces=interfaces if kd == "mindistance" else ())
                 for k, kd in enumerate(kinds))


# ---- inputs of the raw-row tests: name -> (model, loader of (top, center (F, N, 3), quat, box or None), half-charged ends, salt)
def _golden(model, name, frames=10):
    top, traj = H.load_golden(model, name)[:2]
    return top, np.asarray(traj.center[:frames]), np.asarray(traj.quaternions[:frames]), np.broadcast_to(np.asarray(traj.box_size, dtype=np.float64), (3,)).copy()


def _sixty():
    from tests.test_oracle_golden import _sixty_bp

    top, traj, _ = _sixty_bp("simple-helix-60bp-oxdna2")
    return top, np.asarray(traj.center), np.asarray(traj.quaternions), np.broadcast_to(np.asarray(traj.box_size, dtype=np.float64), (3,)).copy()


def _crossing(periodic):
    from tests import oxdna_periodic_synth as S

    top, c, q, box = S.crossing_helix(2, "simple-helix")
    return top, c[None], q[None], (box if periodic else None)


RAW_CASES = {
    "dna1/simple-helix": (1, lambda: _golden(1, "simple-helix"), False, 0.5),
    "dna2/simple-helix": (2, lambda: _golden(2, "simple-helix"), False, 0.5),
    "rna2/simple-helix-12bp": (3, lambda: _golden(3, "simple-helix-12bp"), False, 1.0),
    "regr/simple-helix-60bp-oxdna2": (2, _sixty, True, 0.5),
    "crossing-helix-free": (2, lambda: _crossing(False), False, 0.5),
    "crossing-helix-periodic": (2, lambda: _crossing(True), False, 0.5),
}


@functools.lru_cache(maxsize=None)
def raw_case(name):
    """dict of one raw-row input: model, top, center, quat, box, ops (bond + mindistance over every native pair), the
    oracle's parameters and its rows hb / dist (F, 2 n_bp) - computed once, read-only."""
    model, load, hce, salt = RAW_CASES[name]
    top, c, q, box = load()
    n = int(top.n_nucleotides)
    ops = native_ops(n // 2)
    P = H.oracle_params(model, half_charged_ends=hce, salt=salt)
    hb, dist = oracle_rows(model, P, top.seq, c, q, all_pairs(ops), box=box)
    hb.setflags(write=False)
    dist.setflags(write=False)
    return dict(model=model, top=top, center=c, quat=q, box=box, ops=ops, hce=hce, salt=salt, hb=hb, dist=dist)


def bounds(ref, fp64: bool) -> np.ndarray:
    """The project's comparison bound of a per-pair row against the oracle (tests/test_gpu_oxdna_energy.py): fp64 within
    rtol 1e-9 + atol 1e-11, fp32 within 1e-3 of the largest magnitude of the row set."""
    ref = np.asarray(ref)
    return 1e-9 * np.abs(ref) + 1e-11 if fp64 else np.full(ref.shape, 1e-3 * np.abs(ref).max())
