"""What tests/test_gpu_energy_shapes.py and tests/test_oxdna_energy_shapes_cpu.py share (NumPy and the CPU oracle only):
the systems of the segmented-walk tests with their row layout, segment caps and oracle results, and the frame-chunk
cases with the two chunk rules of the library restated as plain arithmetic.

Systems: the five of ``oxdna_periodic_synth.CROSSING`` - the golden helices of the four models and the ring - each "mid"
(as stored, in the middle of its 20-unit box, where the minimum image subtracts nothing) and "crossing" (the same frames
displaced by ``oxdna_periodic_synth.placement``'s lattice vectors: every pair between the strands goes through an
image), three frames each; and the 120-nt oxDNA2 duplex, frame 0 and the same frame translated.

Rows: ``rows_of`` restates ``set_neighbors`` (mythos_amd/csrc/neighbors.hip, rows_from_pairs): the four bonded slots
first, then the entries in pair-list order - pair (i, j) puts j into row i and i | ROLE_Q into row j - and a stride of
the next multiple of 16 at or above the longest row.  A row LENGTH counts the bonded slots.  ``caps`` derives the
segment sizes from the lengths: 8 (the smallest the hook takes), interior length - 4 (interior rows are exactly one
full segment, end rows get a tail of one entry), end length - 4 (end rows exactly full), 0 (unsegmented, the control).

Chunk rules: ``energy_chunk`` is launch_typed's (mythos_amd/csrc/oxdna_energy_core.inc), ``sweep_chunk`` sweep_typed's
(mythos_amd/csrc/debye_sweep.hip).  The tests assert that their frame counts exceed them: a changed rule makes the
premise fail instead of letting the test pass with one chunk.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

from mythos_amd.input import defaults
from mythos_amd.input import sequence_constraints as scm
from oracle import oxdna_oracle as orc
from tests import helpers as H
from tests import oxdna_periodic_synth as S

SYSTEMS = S.CROSSING
PLACES = ("mid", "crossing")
# Frame 0 and two of the frames tests/test_gpu_oxdna_energy.py::test_forces_and_quaternion_gradients holds the raw dU/dq of, whose
# bounds are used here.  (Not any frame will do in fp32: on frame 41 of the oxRNA2 helix nucleotide 20 sits on a clamp of the
# reference's energy, where the rounding of one fp32 dot product decides the branch; dU/dq then differs from the fp64 oracle by
# 4.5e-3 of its largest component, all of it ALONG q - the part perpendicular to q, which is what moves a body, agrees to 2.2e-4 -
# with and without segments alike.  tests/test_gpu_oxdna_energy.py has the same effect on the hairpin files.)
FRAMES = (0, 17, 42)
PSEQ_MODELS = (1, 2, 4)
LONG = "simple-helix-60bp-oxdna2"
LONG_SHIFT = np.array([0.5, -0.25, 1.0])  # the second frame of the 120-nt case: frame 0 moved rigidly

ROLE_Q = 1 << 30
BONDED_SLOTS = 4
TILE = 32            # nucleotides per workgroup of the energy and the sweep kernel
CAP_MIN, CAP_MAX = 8, 192
N_TERMS = 8
INTERACTS = 1e-6     # a pair interacts if the oracle energy changes by more than this without it

# sequence-dependent weight tables of the oxDNA1 / oxDNA2 cases: with the average-sequence tables the stacking weight
# does not depend on the distribution at all (the construction of tests/test_gpu_pseq.py)
_rng = np.random.default_rng(5)
W_ST, W_HB = _rng.random((4, 4)) + 0.5, _rng.random((4, 4)) + 0.2
BPS = {16: np.array([[1, 14], [2, 13], [5, 10], [7, 8]])}


def system_id(model, name):
    return f"{H.model_dir(model)}-{name}"


# ---- systems ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(model: int, name: str):
    from mythos_amd.input import topology

    if model == 4:
        top, traj, _, _ = H.load_golden_na1(name)
    elif name == "circular":
        ref_top, traj, _, _ = H.load_golden(2, "simple-helix")
        top = topology.from_arrays(ref_top.seq, ref_top.strand_counts, is_circular=[True, False])
    elif name == LONG:
        from tests.test_oracle_golden import _sixty_bp

        top, traj, _ = _sixty_bp(name)
    else:
        top, traj, _, _ = H.load_golden(model, name)
    return top, traj


def half_charged_ends(name):
    return name == LONG


def box_of(model, name):
    return np.broadcast_to(np.asarray(_golden(model, name)[1].box_size, dtype=np.float64), (3,)).copy()


def system_frames(model: int, name: str, place: str):
    """(topology, centres (F, N, 3), quaternions (F, N, 4), box (3,)) in float64: FRAMES of the golden trajectory, for
    "crossing" displaced nucleotide by nucleotide as frame 0 is in oxdna_periodic_synth.crossing_helix."""
    top, traj = _golden(model, name)
    if name == LONG:
        c0, q0 = np.array(traj.center[0], dtype=np.float64), np.array(traj.quaternions[0], dtype=np.float64)
        return top, np.stack([c0, c0 + LONG_SHIFT]), np.stack([q0, q0]), box_of(model, name)
    idx = list(FRAMES)
    c, q = np.array(traj.center[idx], dtype=np.float64), np.array(traj.quaternions[idx], dtype=np.float64)
    if place == "crossing":
        c = c + S.placement(model, name)[4][None]
    return top, c, q, box_of(model, name)


def pair_list(top):
    """The topology's all-pairs list (``top.unbonded_neighbors``), last pair first.  The oracle does not care about the
    order; the rows do: in the topology's own order the single-entry tail of the ring's end rows holds no pair that needs
    an image, reversed every system has one in a later segment (tests/test_oxdna_energy_shapes_cpu.py)."""
    return np.ascontiguousarray(np.asarray(top.unbonded_neighbors, dtype=np.int64).reshape(-1, 2)[::-1])


# ---- rows and segments ---------------------------------------------------------------------------------------------------
def rows_of(top, pairs):
    """(rows (n, stride), lengths (n,)) as set_neighbors lays them out; empty places hold -1."""
    n = int(top.n_nucleotides)
    partners = np.full((n, BONDED_SLOTS), -1, dtype=np.int64)
    for i, j in np.asarray(top.bonded_neighbors).reshape(-1, 2):  # mythos_oxdna_create: i takes an odd slot, j an even one
        si = 1 if partners[i, 1] == -1 else 3
        sj = 0 if partners[j, 0] == -1 else 2
        partners[i, si], partners[j, sj] = j, i
    count = np.bincount(np.asarray(pairs).reshape(-1), minlength=n)
    stride = (int(count.max()) + BONDED_SLOTS + 15) // 16 * 16
    rows = np.full((n, stride), -1, dtype=np.int64)
    rows[:, :BONDED_SLOTS] = partners
    lens = np.full(n, BONDED_SLOTS, dtype=np.int64)
    for i, j in np.asarray(pairs):
        rows[i, lens[i]] = j
        lens[i] += 1
        rows[j, lens[j]] = i | ROLE_Q
        lens[j] += 1
    return rows, lens


def caps(lens):
    """Segment sizes of a system from its row lengths: (8, interior - 4, end - 4, 0), duplicates dropped; ``interior``
    is the shortest row (two bonded partners), ``end`` the longest (one)."""
    out = []
    for cap in (CAP_MIN, int(lens.min()) - BONDED_SLOTS, int(lens.max()) - BONDED_SLOTS, 0):
        if cap not in out:
            out.append(cap)
    return tuple(out)


def long_caps(lens):
    return (CAP_MIN, int(lens.min()) - BONDED_SLOTS)


def segments(length: int, cap: int):
    """[(first, end)] of a row of ``length`` walked with ``cap`` entries per segment (gather_row); cap 0: one segment."""
    if cap == 0:
        return [(BONDED_SLOTS, length)] if length > BONDED_SLOTS else []
    return [(s, min(length, s + cap)) for s in range(BONDED_SLOTS, length, cap)]


def is_segmented(stride: int, cap: int) -> bool:
    """launch_typed: the hook only ever shortens the lists, and the walk is segmented when the stride exceeds them."""
    return cap != 0 and stride > min(stride, CAP_MAX, cap)


# ---- oracle --------------------------------------------------------------------------------------------------------------
def leaf_cfg(model):
    """(sim, sections, {key: leaf}) with every non-geometry scalar a torch leaf; oxNA: the three sets, keys (set, section,
    name) - tests/test_gpu_oxdna_energy.py::_leaf_cfg and tests/test_gpu_na1.py::_leaf_cfgs."""
    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    leaves = {}
    for which, sections in (cfg.items() if model == 4 else (("", cfg),)):
        for sec, d in sections.items():
            if sec == "geometry":
                continue
            for k, v in d.items():
                d[k] = leaves[(which, sec, k)] = torch.tensor(float(v), dtype=torch.float64, requires_grad=True)
    _weights(model, cfg)
    return sim, cfg, leaves


def _weights(model, cfg):
    if model in (1, 2):
        cfg["stacking"]["ss_stack_weights"] = torch.as_tensor(W_ST)
        cfg["hydrogen_bonding"]["ss_hb_weights"] = torch.as_tensor(W_HB)


def plain_cfg(model):
    sim, cfg = defaults.default_configs_for(H.model_dir(model))
    _weights(model, cfg)
    return sim, cfg


def constraints(n):
    return scm.from_bps(n, BPS[n])


def soft_distribution(n):
    """(unpaired (U, 4), base pairs (B, 4)) rows of probabilities, none of them near one-hot."""
    sc = constraints(n)
    rng = np.random.default_rng(11)

    def dist(rows):
        a = rng.random((rows, 4)) + 0.05
        return a / a.sum(1, keepdims=True)

    return dist(sc.n_unpaired), dist(sc.n_bp)


def oracle_params(model, name, cfg, kt, pseq=None):
    if pseq is not None:
        sc = constraints(pseq[0].shape[0] + 2 * pseq[1].shape[0])
        for sections in (cfg.values() if model == 4 else (cfg,)):
            for sec in ("hydrogen_bonding",) if model == 4 else ("stacking", "hydrogen_bonding"):
                sections[sec].update(pseq=pseq, pseq_constraints=sc)
    if model == 4:
        return orc.init_all_na1(cfg["dna"], cfg["rna"], cfg["drh"], kt=kt, salt_conc=S.SALT[4], half_charged_ends=False)
    return orc.init_all(model, cfg, kt=kt, salt_conc=S.SALT[model], half_charged_ends=half_charged_ends(name))


def _topo(top, pairs):
    return (torch.as_tensor(top.seq, dtype=torch.long), torch.as_tensor(top.is_end, dtype=torch.long),
            torch.as_tensor(np.asarray(top.bonded_neighbors), dtype=torch.long).reshape(-1, 2), torch.as_tensor(pairs, dtype=torch.long).reshape(-1, 2))


def oracle_terms(model, P, top, c, q, pairs, box):
    """(8,) term energies with the graph of whatever ``P``, ``c``, ``q`` carry (oxDNA1: seven terms, the eighth 0)."""
    seq, is_end, b, u = _topo(top, pairs)
    ct, qt = torch.as_tensor(c), torch.as_tensor(q)
    if model == 4:
        return orc.energy_terms_na1(P, ct, qt, seq, torch.as_tensor(S.is_rna(top)), is_end, b, u, box=box)
    e = orc.energy_terms(model, P, ct, qt, seq, is_end, b, u, box=box)
    return torch.cat([e, e.new_zeros(N_TERMS - e.shape[0])])


def oracle_grads(model, P, top, c, q, pairs, box):
    seq, is_end, b, u = _topo(top, pairs)
    ct, qt = torch.as_tensor(c), torch.as_tensor(q)
    if model == 4:
        return orc.energy_and_grads_na1(P, ct, qt, seq, torch.as_tensor(S.is_rna(top)), is_end, b, u, box=box)
    return orc.energy_and_grads(model, P, ct, qt, seq, is_end, b, u, box=box)


def pair_energies(model, name, top, c, q, pairs, box):
    """(P,) oracle energy of every listed pair, all terms added: what the total changes by when the pair leaves the list."""
    sim, cfg = plain_cfg(model)
    P = oracle_params(model, name, cfg, sim["kT"])
    seq, is_end, b, u = _topo(top, pairs)
    ct, qt = torch.as_tensor(c), torch.as_tensor(q)
    if model == 4:
        _, ut = orc.pair_terms_na1(P, ct, qt, seq, torch.as_tensor(S.is_rna(top)), is_end, b, u, box=box)
    else:
        _, ut = orc.pair_terms(model, P, ct, qt, seq, is_end, b, u, box=box)
    return sum(ut.values()).detach().numpy()


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle(model: int, name: str, place: str, frames=None):
    """Per frame of ``system_frames`` (or of the synthetic frames ``frames``, a tuple of indices): terms (F, 8), dU/dc,
    dU/dq, dU/dtheta (F, leaves + kT) by autograd through an independent ``init_all``, and - models with a probabilistic
    sequence - the terms under ``soft_distribution`` with dU/d(unpaired), dU/d(base pairs).  Read-only arrays."""
    if frames is None:
        top, c, q, box = system_frames(model, name, place)
    else:
        top, c, q, box = synthetic_frames(model, name, place, np.asarray(frames))
    pairs = pair_list(top)
    sim, cfg = plain_cfg(model)
    P = oracle_params(model, name, cfg, sim["kT"])
    sim_l, cfg_l, leaves = leaf_cfg(model)
    kt = torch.tensor(sim_l["kT"], dtype=torch.float64, requires_grad=True)
    P_l = oracle_params(model, name, cfg_l, kt)
    out = {"terms": [], "gc": [], "gq": [], "dtheta": [], "keys": list(leaves) + ["kt"]}
    soft = model in PSEQ_MODELS and name != LONG
    if soft:
        up, bp = (torch.tensor(a, requires_grad=True) for a in soft_distribution(int(top.n_nucleotides)))
        sim_s, cfg_s = plain_cfg(model)
        P_s = oracle_params(model, name, cfg_s, sim_s["kT"], pseq=(up, bp))
        out.update(soft_terms=[], g_up=[], g_bp=[])
    for f in range(c.shape[0]):
        out["terms"].append(oracle_terms(model, P, top, c[f], q[f], pairs, box).detach().numpy())
        _, gc, gq = oracle_grads(model, P, top, c[f], q[f], pairs, box)
        out["gc"].append(gc.numpy())
        out["gq"].append(gq.numpy())
        u = oracle_terms(model, P_l, top, c[f], q[f], pairs, box).sum()
        g = torch.autograd.grad(u, [*leaves.values(), kt], retain_graph=True, allow_unused=True)
        out["dtheta"].append(np.array([0.0 if x is None else float(x) for x in g]))
        if soft:
            e = oracle_terms(model, P_s, top, c[f], q[f], pairs, box)
            g_up, g_bp = torch.autograd.grad(e.sum(), [up, bp], retain_graph=True)
            out["soft_terms"].append(e.detach().numpy())
            out["g_up"].append(g_up.numpy())
            out["g_bp"].append(g_bp.numpy())
    return {k: (v if k == "keys" else _frozen(np.stack(v))) for k, v in out.items()}


# ---- frame chunks --------------------------------------------------------------------------------------------------------
TAIL = 70            # frames past the first chunk
GRID_Y = 65535
ENERGY_SCRATCH = 256 << 20
SWEEP_SCRATCH = 64 << 20
SWEEP_MAX_T = 128
SWEEP_CONSTS = 5
NOISE_C = NOISE_Q = 0.01
KT_LOW = 1e-4        # (tests/test_gpu_melting.py) r_cut of the Debye-Hueckel term is about 0.06 there: a row of zeros


def param_count() -> int:
    from mythos_amd import _lib

    return int(_lib.load().mythos_oxdna_param_count())


def energy_chunk(n: int, param_grads: bool, param_sets: int = 1) -> int:
    """Frames per launch of an energy call: launch_typed's rule."""
    blocks = -(-n // TILE)
    width = param_sets * param_count() if param_grads else N_TERMS
    return min(GRID_Y, max(1, ENERGY_SCRATCH // (blocks * width * 8)))


def sweep_chunk(n: int, n_kt: int, const_grads: bool) -> int:
    """Frames per launch of a Debye-Hueckel sweep: sweep_typed's rule."""
    tiles = -(-n // TILE)
    width = 1 + SWEEP_CONSTS if const_grads else 1
    return min(GRID_Y, max(1, SWEEP_SCRATCH // (tiles * min(n_kt, SWEEP_MAX_T) * width * 8)))


def synthetic_frames(model: int, name: str, place: str, index):
    """(topology, centres, quaternions, box) of the synthetic frames ``index`` (an array of frame numbers, or a count F for
    0 .. F - 1): frame k is golden frame k mod 100 (mod the length of a shorter trajectory), centres displaced by
    N(0, 0.01^2) noise, quaternions perturbed likewise and renormalised, from the generator seeded with k // 100 - a
    frame is the same whichever call asks for it."""
    top, traj = _golden(model, name)
    index = np.arange(index) if np.ndim(index) == 0 else np.asarray(index, dtype=np.int64)
    n, n_gold = int(top.n_nucleotides), int(traj.center.shape[0])
    blocks = np.unique(index // 100)
    noise = np.empty((len(blocks), 100, n, 7))
    for k, b in enumerate(blocks):
        noise[k] = np.random.default_rng(int(b)).standard_normal((100, n, 7))
    at = noise[np.searchsorted(blocks, index // 100), index % 100]
    gold = (index % 100) % n_gold
    c = np.asarray(traj.center, dtype=np.float64)[gold] + NOISE_C * at[..., :3]
    q = np.asarray(traj.quaternions, dtype=np.float64)[gold] + NOISE_Q * at[..., 3:]
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    if place == "crossing":
        c += S.placement(model, name)[4][None]
    return top, c, q, box_of(model, name)


def boundary_frames(chunk: int, n_frames: int):
    """The frames the oracle sees: both sides of the chunk boundary, the first, the last, one in the middle of the tail."""
    return tuple(sorted({0, *range(chunk - 2, chunk + 3), chunk + TAIL // 2, n_frames - 1}))


def slices(chunk: int, n_frames: int):
    """Calls of their own whose results the whole call must reproduce bit for bit."""
    return (slice(0, 100), slice(chunk - 50, chunk + 50), slice(n_frames - TAIL, n_frames))


def sweep_kts(own_kt: float):
    """129 temperatures = two passes of the sweep (128 + 1): the function's own kT first, KT_LOW last in the first pass,
    and a temperature with a live Debye-Hueckel term alone in the second."""
    return np.concatenate([[own_kt], np.linspace(0.09, 0.12, 126), [KT_LOW, 0.105]])


SWEEP_T_ORACLE = (0, 1, 32, 64, 96, 127, 128)
# temperature slices that see the same packed pair list as the whole call: a pass keeps the pairs inside the LARGEST
# r_cut of its temperatures (index 126, kT = 0.12, in the first pass), and the order of the 64-lane sums follows the list
SWEEP_T_SLICES = ((0, 1, 64, 126, 127), (128,))
